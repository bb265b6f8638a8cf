// hip_own_check.cpp -- the owning handles of azdopt_amd/csrc/hip_own.h on their own: `no-device` walks every failure path (where
// no device is visible every acquisition fails), `device` every success path.  Exit 0: all checks held; 1: one did not (named on
// stderr); 77: the mode does not fit this machine.  Built by tests/test_hip_own.py and tests/test_gpu_hip_own.py.
#include "../../azdopt_amd/csrc/hip_own.h"

#include <cstdio>
#include <cstring>

namespace azd {
thread_local std::string g_last_error;
int hip_fail(hipError_t e, const char *what) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorNoDevice || e == hipErrorInvalidDevice ? AZD_ERR_NO_DEVICE : e == hipErrorOutOfMemory ? AZD_ERR_OUT_OF_MEMORY : AZD_ERR_HIP;
}
} // namespace azd
using namespace azd;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "line %d: %s does not hold (last error: %s)\n", __LINE__, #cond, g_last_error.c_str()); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

// moves of empty handles, one onto itself included, and reset() call nothing and leave them empty
template <typename H>
static int empty_moves() {
    H a, b(std::move(a));
    a = std::move(b);
    H &self = a;
    a = std::move(self);
    a.reset();
    CHECK(a.empty() && b.empty() && !a.get() && !b.get());
    return 0;
}

static int no_device() {
    DevBuf<float> d;
    CHECK(d.alloc(1024) != AZD_OK && d.empty() && !d.get() && d.count() == 0 && !g_last_error.empty());
    CHECK(d.alloc(0) == AZD_OK && d.empty()); // nothing is asked for: nothing can fail
    Pinned<uint32_t> h, hc;
    CHECK(h.alloc(16) != AZD_OK && h.empty() && h.count() == 0);
    CHECK(hc.alloc(16, hipHostMallocCoherent) != AZD_OK && hc.empty() && hc.count() == 0);
    Stream s;
    CHECK(s.create() != AZD_OK && s.empty());
    CHECK(s.create(hipStreamNonBlocking) != AZD_OK && s.empty());
    Event ev;
    CHECK(ev.create() != AZD_OK && ev.empty());
    CHECK(ev.create(hipEventDisableTiming) != AZD_OK && ev.empty());
    GraphExec g;
    g.adopt(nullptr);
    CHECK(g.empty() && !g.get());
    {
        DevArena arena;
        int marker = 0, *p = &marker;
        CHECK(arena.alloc(&p, 64) != AZD_OK && p == &marker && arena.size() == 0);
    }
    DevBuf<float> a, b;
    Pinned<float> c;
    DevBuf<uint16_t> e;
    const int st = alloc_set(a, 8, b, 8, c, 8, e, 8);
    CHECK(st != AZD_OK && st == d.alloc(8)); // the first failure's status
    CHECK(a.empty() && b.empty() && c.empty() && e.empty());
    CHECK(alloc_set() == AZD_OK);
    CHECK(empty_moves<DevBuf<double>>() == 0 && empty_moves<Pinned<int>>() == 0 && empty_moves<Stream>() == 0 && empty_moves<Event>() == 0 &&
          empty_moves<GraphExec>() == 0);
    return 0;
}

// p is device memory of device `dev`, as the runtime sees it.  (The runtime either refuses an address it does not know or
// answers "unregistered" for it: neither is `live`.)
static bool live(const void *p, int dev) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    const bool ok = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == dev;
    (void)hipGetLastError();
    return ok;
}

static int device(int dev) {
    CHECK(hipSetDevice(dev) == hipSuccess);
    DevBuf<float> a;
    CHECK(a.alloc(1024) == AZD_OK && !a.empty() && a.count() == 1024 && live(a.get(), dev));
    const float *old = a;
    a.reset();
    CHECK(a.empty() && a.count() == 0 && !live(old, dev));
    // a move-assignment releases what the target held; the source ends empty
    DevBuf<float> b;
    CHECK(a.alloc(1024) == AZD_OK && b.alloc(2048) == AZD_OK);
    const float *old_a = a, *old_b = b;
    a = std::move(b);
    CHECK(b.empty() && b.count() == 0 && a.get() == old_b && a.count() == 2048 && live(old_b, dev) && !live(old_a, dev));
    DevBuf<float> c(std::move(a));
    CHECK(a.empty() && c.get() == old_b && c.count() == 2048 && live(old_b, dev));
    {
        DevBuf<float> scoped(std::move(c));
        CHECK(c.empty() && scoped.get() == old_b);
    }
    CHECK(!live(old_b, dev)); // destruction
    // a regrow releases the smaller buffer (where the runtime hands the same address out again, the new buffer lives there)
    CHECK(a.alloc(1024) == AZD_OK);
    old = a;
    CHECK(a.alloc(1 << 20) == AZD_OK && a.count() == (1u << 20) && live(a.get(), dev));
    if (a.get() != old) CHECK(!live(old, dev));
    Pinned<uint32_t> h, hc;
    CHECK(h.alloc(16) == AZD_OK && hc.alloc(16, hipHostMallocCoherent) == AZD_OK && h.count() == 16 && !hc.empty());
    h[3] = 7u;
    Pinned<uint32_t> h2(std::move(h));
    CHECK(h.empty() && h2[3] == 7u);
    {
        DevArena arena;
        uint64_t *p = nullptr, *q = nullptr;
        CHECK(arena.alloc(&p, 64) == AZD_OK && arena.alloc(&q, 64) == AZD_OK && p && q && p != q && arena.size() == 2 && live(p, dev));
        old = (const float *)p;
    }
    CHECK(!live(old, dev));
    DevBuf<uint8_t> s1, s2;
    Pinned<float> s3;
    CHECK(alloc_set(s1, 100, s2, 4096, s3, 4) == AZD_OK && s1.count() == 100 && s2.count() == 4096 && s3.count() == 4 && live(s2.get(), dev));
    Stream st, st2;
    CHECK(st.create(hipStreamNonBlocking) == AZD_OK && !st.empty() && st2.create() == AZD_OK);
    CHECK(hipMemsetAsync(s2, 0x5a, 4096, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess);
    uint8_t back[4096];
    CHECK(hipMemcpy(back, s2, 4096, hipMemcpyDeviceToHost) == hipSuccess && back[0] == 0x5a && back[4095] == 0x5a);
    Event ev, ev2;
    CHECK(ev.create(hipEventDisableTiming) == AZD_OK && ev2.create() == AZD_OK && !ev.empty());
    CHECK(hipEventRecord(ev, st) == hipSuccess && hipEventSynchronize(ev) == hipSuccess);
    const hipStream_t raw = st;
    st2 = std::move(st); // (st2's own stream is destroyed)
    CHECK(st.empty() && st2.get() == raw && hipStreamSynchronize(st2) == hipSuccess);
    Event ev3(std::move(ev));
    CHECK(ev.empty() && !ev3.empty() && hipEventQuery(ev3) == hipSuccess);
    // a captured memset, instantiated: the executable is owned, launched and released
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    CHECK(hipStreamBeginCapture(st2, hipStreamCaptureModeThreadLocal) == hipSuccess);
    CHECK(hipMemsetAsync(s2, 0x11, 4096, st2) == hipSuccess);
    CHECK(hipStreamEndCapture(st2, &graph) == hipSuccess && graph);
    const hipError_t hi = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    CHECK(hi == hipSuccess && exec);
    GraphExec g, g2;
    g.adopt(exec);
    g2 = std::move(g);
    CHECK(g.empty() && g2.get() == exec);
    CHECK(hipGraphLaunch(g2, st2) == hipSuccess && hipStreamSynchronize(st2) == hipSuccess);
    CHECK(hipMemcpy(back, s2, 4096, hipMemcpyDeviceToHost) == hipSuccess && back[0] == 0x11 && back[4095] == 0x11);
    g2.reset();
    CHECK(g2.empty() && hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess);
    return 0;
}

int main(int argc, char **argv) {
    const bool want_device = argc > 1 && !strcmp(argv[1], "device");
    if (argc < 2 || (!want_device && strcmp(argv[1], "no-device"))) {
        fprintf(stderr, "usage: %s no-device | device\n", argv[0]);
        return 2;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    if (want_device != (n > 0)) {
        fprintf(stderr, "%d device(s) visible: not the machine for mode %s\n", n, argv[1]);
        return 77;
    }
    const int rc = want_device ? device(0) : no_device();
    if (rc == 0) printf("hip_own_check %s: ok\n", argv[1]);
    return rc;
}

// hip_own.h -- owners of the HIP resources the host side holds: device and pinned memory, streams, events, graph executables.
// Move-only.  An acquisition that fails reports through hip_fail and leaves the handle empty; an empty handle's destructor calls
// nothing (without a device hipFree(nullptr) itself is an error).  A handle reads as the pointer it owns wherever one is expected
// (kernel arguments, copies, offsets).  The release calls of the library stand here and nowhere else.  Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/azdopt_amd.h"

namespace azd {

extern thread_local std::string g_last_error; // defined in engine.hip, as hip_fail is
int hip_fail(hipError_t e, const char *what);

#define AZD_HIP(call)                                        \
    do {                                                     \
        hipError_t _e = (call);                              \
        if (_e != hipSuccess) return azd::hip_fail(_e, #call); \
    } while (0)
// a status that is not AZD_OK ends the calling function (as AZD_HIP does for a HIP call)
#define AZD_ST(call)            \
    do {                        \
        const int st_ = (call); \
        if (st_) return st_;    \
    } while (0)

template <typename T>
class DevBuf { // hipMalloc memory of count() elements
    T *p_ = nullptr;
    size_t n_ = 0;

  public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept { return this == &o ? *this : (reset(std::exchange(o.p_, nullptr), std::exchange(o.n_, 0)), *this); }
    ~DevBuf() { reset(); }
    int alloc(size_t count) { // what the handle holds is released first; count 0: it stays empty
        reset();
        T *p = nullptr;
        const hipError_t e = count ? hipMalloc((void **)&p, count * sizeof(T)) : hipSuccess;
        if (e != hipSuccess) return hip_fail(e, "hipMalloc");
        reset(p, p ? count : 0);
        return AZD_OK;
    }
    void reset(T *p = nullptr, size_t n = 0) {
        if (p_) (void)hipFree(p_);
        p_ = p, n_ = n;
    }
    T *get() const { return p_; }
    size_t count() const { return n_; }
    bool empty() const { return !p_; }
    operator T *() const { return p_; }
};

template <typename T>
class Pinned { // hipHostMalloc memory (flags: hipHostMallocCoherent for what a running kernel hands the host)
    T *p_ = nullptr;
    size_t n_ = 0;

  public:
    Pinned() = default;
    Pinned(Pinned &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    Pinned &operator=(Pinned &&o) noexcept { return this == &o ? *this : (reset(std::exchange(o.p_, nullptr), std::exchange(o.n_, 0)), *this); }
    ~Pinned() { reset(); }
    int alloc(size_t count, unsigned flags = hipHostMallocDefault) {
        reset();
        T *p = nullptr;
        const hipError_t e = count ? hipHostMalloc((void **)&p, count * sizeof(T), flags) : hipSuccess;
        if (e != hipSuccess) return hip_fail(e, "hipHostMalloc");
        reset(p, p ? count : 0);
        return AZD_OK;
    }
    void reset(T *p = nullptr, size_t n = 0) {
        if (p_) (void)hipHostFree(p_);
        p_ = p, n_ = n;
    }
    T *get() const { return p_; }
    size_t count() const { return n_; }
    bool empty() const { return !p_; }
    operator T *() const { return p_; }
    T *operator->() const { return p_; }
};

// Buffers that are allocated together end whole or empty: alloc_set(buf_a, count_a, buf_b, count_b, ...) releases every member,
// allocates them in the order given, and on the first failure releases every member again and returns that failure's status.
inline void reset_set_() {}
template <typename B, typename... R>
void reset_set_(B &b, size_t, R &...r) { b.reset(), reset_set_(r...); }
inline int alloc_set_() { return AZD_OK; }
template <typename B, typename... R>
int alloc_set_(B &b, size_t count, R &...r) {
    const int st = b.alloc(count);
    return st ? st : alloc_set_(r...);
}
template <typename... A>
int alloc_set(A &&...a) {
    reset_set_(a...);
    const int st = alloc_set_(a...);
    if (st) reset_set_(a...);
    return st;
}

class DevArena { // device allocations of one fixed lifetime, handed out as raw pointers (what a kernel takes by value points into it)
    std::vector<void *> v_;

  public:
    DevArena() = default;
    DevArena(const DevArena &) = delete;
    DevArena &operator=(const DevArena &) = delete;
    ~DevArena() {
        for (void *p : v_) (void)hipFree(p);
    }
    template <typename T>
    int alloc(T **p, size_t count) { // *p is written on success only
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, count * sizeof(T));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc");
        if (q) v_.push_back(q);
        *p = (T *)q;
        return AZD_OK;
    }
    size_t size() const { return v_.size(); }
};

class Stream {
    hipStream_t s_ = nullptr;

  public:
    Stream() = default;
    Stream(Stream &&o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream &operator=(Stream &&o) noexcept { return this == &o ? *this : (adopt(std::exchange(o.s_, nullptr)), *this); }
    ~Stream() { reset(); }
    int create(unsigned flags = hipStreamDefault) {
        hipStream_t s = nullptr;
        const hipError_t e = hipStreamCreateWithFlags(&s, flags);
        if (e != hipSuccess) return hip_fail(e, "hipStreamCreate");
        adopt(s);
        return AZD_OK;
    }
    void adopt(hipStream_t s) {
        if (s_) (void)hipStreamDestroy(s_);
        s_ = s;
    }
    void reset() { adopt(nullptr); }
    hipStream_t get() const { return s_; }
    bool empty() const { return !s_; }
    operator hipStream_t() const { return s_; }
};

class Event {
    hipEvent_t e_ = nullptr;

  public:
    Event() = default;
    Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event &operator=(Event &&o) noexcept { return this == &o ? *this : (adopt(std::exchange(o.e_, nullptr)), *this); }
    ~Event() { reset(); }
    int create(unsigned flags = hipEventDefault) {
        hipEvent_t ev = nullptr;
        const hipError_t e = hipEventCreateWithFlags(&ev, flags);
        if (e != hipSuccess) return hip_fail(e, "hipEventCreate");
        adopt(ev);
        return AZD_OK;
    }
    void adopt(hipEvent_t ev) {
        if (e_) (void)hipEventDestroy(e_);
        e_ = ev;
    }
    void reset() { adopt(nullptr); }
    hipEvent_t get() const { return e_; }
    bool empty() const { return !e_; }
    operator hipEvent_t() const { return e_; }
};

class GraphExec { // an instantiated graph: adopt() takes over what hipGraphInstantiate returned
    hipGraphExec_t g_ = nullptr;

  public:
    GraphExec() = default;
    GraphExec(GraphExec &&o) noexcept : g_(std::exchange(o.g_, nullptr)) {}
    GraphExec &operator=(GraphExec &&o) noexcept { return this == &o ? *this : (adopt(std::exchange(o.g_, nullptr)), *this); }
    ~GraphExec() { reset(); }
    void adopt(hipGraphExec_t g) {
        if (g_) (void)hipGraphExecDestroy(g_);
        g_ = g;
    }
    void reset() { adopt(nullptr); }
    hipGraphExec_t get() const { return g_; }
    bool empty() const { return !g_; }
    operator hipGraphExec_t() const { return g_; }
};

} // namespace azd

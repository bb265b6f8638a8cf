// gemm_f32_gathered.inc -- included by mlp_kernels.hip (inside namespace azd).
//
// The fp32 evaluator of the searcher-only pool step (engine_rollout.hip: ext_pool_run under AZD_ENGINE_EXT_POOL_F32): one layer
// Y = act(A . W^T + b) over a row list whose length lives in device memory, on v_mfma_f32_32x32x2_f32.  The EXT conventions of
// k_gemm16<BN, true> (gemm_bf16_glds.inc): the row count is *m_dev clamped to max_rows, the grid is sized for max_rows and the
// blocks beyond the tiles of *m_dev rows leave at once (a count of 0: nothing happens), row i of A is row rows_in[i] of the array
// behind A (null: row i), row i of Y goes to row rows_out[i] (null: row i); rows no list entry names are not written.  Rows are
// read with plain loads and written with plain stores: the searchers' rows are written through and a launch acquires, its end
// releases (pool_step.inc, "searchers only").
//
// Summation contract: every output element is acc = fmaf(a[k], w[k], acc) for k = 0 .. K - 1 ascending from +0.0f, then + bias,
// then the activation with k_gemm's EPI_BIAS_ACT expressions (expf, IEEE division) -- the sums of forward(quant = false) through
// k_gemm<true, true>, bit for bit (tests/test_gpu_gemm_f32_gathered.py), whichever rows share a tile.  So: the same MFMA, the same
// lane -> k mapping (step s multiplies k = 2 s and 2 s + 1), no split of K, and as many zero-padded steps behind K as k_gemm runs
// (it pads K to a multiple of 16: a step of zeros turns an accumulator of -0.0f into +0.0f).
//
// The dense-graph space's pool step asks for the same evaluator (the flag alone on AZD_SPACE_DENSE): S = 3 E + 1 is a multiple of 4
// only when E = 1 (mod 4) -- N = 31 and N = 50 take VEC, N = 8, 20, 33 and 64 the one-float path -- rows are 0/1-valued but for the
// last entry, heads run from 56 to 4032 columns; nothing in the kernel or its launcher had to change for them
// (tests/test_gpu_gemm_f32_gathered_dense.py).
//
// Shape: a batch is tens to a few hundred rows against K of 1380 .. 5049, and the chain above is K / 2 dependent MFMAs of 16
// passes whatever the tile -- a wave alone nearly fills its SIMD's matrix pipe, so the grid is many small tiles: a block is 256
// threads = 4 waves, one per SIMD, over 32 rows x 128 columns; the 32-row A panel is staged once and shared by the four waves,
// each wave owns 32 columns (one 32 x 32 accumulator).  What is left to win is keeping that chain going, so nothing may stand
// between two tiles' MFMAs:
//   * a k tile is 64 wide (32 MFMAs, ~2000 cycles: more than a load that misses the L2 takes); tile t + 2's global loads are
//     issued during tile t's MFMAs and land in registers;
//   * two LDS buffers (separate arrays, so that hipcc knows a write to one cannot alias a read of the other): tile t + 1's
//     registers are written to the other buffer DURING tile t's MFMAs -- a quarter of the writes and of the loads in front of
//     each quarter of the MFMAs, held there by scheduling barriers -- and one block barrier per tile is left.  (Built first:
//     one buffer, stash / barrier / loads / MFMAs / barrier -- the stores, the loads' address arithmetic and the two barriers
//     stood between the tiles' chains, 1.7 us per tile where the MFMAs are 1.0.)
//   * 87 KB of LDS: one block per CU, on purpose.  The evaluator's two streams run the same layers side by side, and two
//     blocks on a CU share its four matrix pipes: each takes twice as long (measured on the one-buffer form padded to 81 KB:
//     r45 0.87 -> 0.97 M expansions/s, r3333 0.89 -> 0.93).
// LDS image: row-major with a 68-float pitch, k permuted inside the tile so that position 32 (k & 1) + (k >> 1) holds k: lane
// (i, h) then reads its 32 operands of a tile -- k = h, h + 2, .. -- as eight 16-byte ds_reads, and a staged float4 leaves as
// two 8-byte ds_writes.
// VEC: K, both pitches and both base addresses are multiples of 4 floats: 16-byte global loads.  Otherwise (r3333's first layer:
// state rows and weight rows of pitch 5049) rows start anywhere: one float per lane and load, 64 consecutive k per wave, so
// that every load instruction still covers whole 128-byte lines where k_gemm's fallback reads four scalars per lane.
constexpr int GF_BM = 32, GF_BN = 128, GF_BK = 64, GF_LD = GF_BK + 4;

template <bool VEC>
__global__ __launch_bounds__(256) void k_gemm_f32_gathered(const float *__restrict__ A, const int lda, const float *__restrict__ W, const int ldw,
                                                           float *__restrict__ Y, const int ldy, const int max_rows, const int N, const int K, const int act,
                                                           const float *__restrict__ bias, const uint32_t *__restrict__ m_dev,
                                                           const uint32_t *__restrict__ rows_in, const uint32_t *__restrict__ rows_out) {
    int M = max_rows;
    if (m_dev) {
        const uint32_t m = *m_dev;
        M = m < (uint32_t)M ? (int)m : M;
    }
    if (M <= 0) return;
    const int nbn = (N + GF_BN - 1) / GF_BN;
    const int bm = (int)blockIdx.x / nbn, bn = (int)blockIdx.x - bm * nbn;
    const int m0 = bm * GF_BM, n0 = bn * GF_BN;
    if (m0 >= M) return;
    __shared__ __attribute__((aligned(16))) float sA0[GF_BM * GF_LD];
    __shared__ __attribute__((aligned(16))) float sW0[GF_BN * GF_LD];
    __shared__ __attribute__((aligned(16))) float sA1[GF_BM * GF_LD];
    __shared__ __attribute__((aligned(16))) float sW1[GF_BN * GF_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // staging.  VEC: thread t moves the float4 at k = 4 (t & 15) of rows (t >> 4) + 16 q -- q < 2 of A, q < 8 of W; else the float
    // at k = t & 63 of rows (t >> 6) + 4 q -- q < 8 of A, q < 32 of W: NU = 10 / 40 units (a unit: one load, its registers, its
    // LDS writes), dealt to the four quarters of a tile.  Every load is unconditional on a clamped address -- rows past M read
    // row M - 1 and columns past N row N - 1 (never stored), k past K reads k = 0 and is replaced by zero on its way into LDS
    // (not where it is loaded: the select would wait for the load) -- so that the loop holds no branch around a load: a load
    // behind a branch is waited for where it is issued.
    constexpr int PER = VEC ? 4 : 1;                  // floats per load
    constexpr int RSTEP = 256 * PER / GF_BK;          // rows the block covers per load: 16 / 4
    constexpr int AQ = GF_BM / RSTEP, WQ = GF_BN / RSTEP, NU = AQ + WQ;
    const int tk = (tid % (GF_BK / PER)) * PER, tr = tid / (GF_BK / PER);
    size_t a_off[AQ];
#pragma unroll
    for (int q = 0; q < AQ; ++q) {
        int row = m0 + tr + RSTEP * q;
        row = row < M ? row : M - 1;
        a_off[q] = (rows_in ? (size_t)rows_in[row] : (size_t)row) * (size_t)lda;
    }
    float reg[NU * PER];
    // units u with u * 4 / NU == g (g = 0 .. 3; g < 0: all of them)
    auto fetch = [&](const int k0, const int g) __attribute__((always_inline)) {
        const int kc = k0 + tk < K ? k0 + tk : 0; // (VEC: K is a multiple of 4, a quad is inside or outside as a whole)
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (g >= 0 && u * 4 / NU != g) continue;
            const float *p;
            if (u < AQ) p = A + a_off[u < AQ ? u : 0] + kc;
            else {
                int row = n0 + tr + RSTEP * (u - AQ);
                row = row < N ? row : N - 1;
                p = W + (size_t)row * (size_t)ldw + kc;
            }
            if constexpr (VEC) {
                const float4 v = *reinterpret_cast<const float4 *>(p);
                reg[4 * u] = v.x, reg[4 * u + 1] = v.y, reg[4 * u + 2] = v.z, reg[4 * u + 3] = v.w;
            } else {
                reg[u] = *p;
            }
        }
    };
    auto stash = [&](float *dA, float *dW, const int k0, const int g) __attribute__((always_inline)) {
        const bool k_ok = k0 + tk < K;
        const int pos = VEC ? (tk >> 1) : (tk & 1) * (GF_BK / 2) + (tk >> 1); // VEC: k = tk .. tk + 3 -> tk / 2, 32 + tk / 2, tk / 2 + 1, 32 + tk / 2 + 1
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (g >= 0 && u * 4 / NU != g) continue;
            float *d = (u < AQ ? dA + (tr + RSTEP * u) * GF_LD : dW + (tr + RSTEP * (u - AQ)) * GF_LD) + pos;
            if constexpr (VEC) {
                *reinterpret_cast<float2 *>(d) = k_ok ? make_float2(reg[4 * u], reg[4 * u + 2]) : make_float2(0.f, 0.f);
                *reinterpret_cast<float2 *>(d + GF_BK / 2) = k_ok ? make_float2(reg[4 * u + 1], reg[4 * u + 3]) : make_float2(0.f, 0.f);
            } else {
                *d = k_ok ? reg[u] : 0.f;
            }
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // lane l feeds A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31], as in k_gemm; 16 k = 8 MFMAs at a time
    const int li = lane & 31, lk = lane >> 5;
    const int fa_off = li * GF_LD + lk * (GF_BK / 2), fw_off = (wave * 32 + li) * GF_LD + lk * (GF_BK / 2);
    auto part = [&](const float *cA, const float *cW, const int h) __attribute__((always_inline)) {
        const float *fa = cA + fa_off + 8 * h, *fw = cW + fw_off + 8 * h;
        const float4 a0 = *reinterpret_cast<const float4 *>(fa), a1 = *reinterpret_cast<const float4 *>(fa + 4);
        const float4 b0 = *reinterpret_cast<const float4 *>(fw), b1 = *reinterpret_cast<const float4 *>(fw + 4);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b0.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b0.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b0.w, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b1.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b1.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b1.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b1.w, acc, 0, 0, 0);
    };
    // k_gemm's k tiles are 16 wide: it runs the MFMA steps below K16 = K rounded up to 16, and so does this kernel: `full` whole
    // tiles, then `tail` sixteenths of one more
    const int K16 = (K + 15) & ~15, full = K16 / GF_BK, tail = (K16 % GF_BK) / 16;
    // a whole tile t in (cA, cW); the registers hold tile t + 1 and go to (nA, nW), tile t + 2 comes into the registers
    auto step = [&](const float *cA, const float *cW, float *nA, float *nW, const int t) __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            stash(nA, nW, (t + 1) * GF_BK, g);
            fetch((t + 2) * GF_BK, g);
            part(cA, cW, g);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads(); // tile t + 1 is written by every wave, tile t read by all
    };
    fetch(0, -1);
    stash(sA0, sW0, 0, -1);
    fetch(GF_BK, -1);
    __syncthreads();
    int t = 0;
    for (; t + 2 <= full; t += 2) {
        step(sA0, sW0, sA1, sW1, t);
        step(sA1, sW1, sA0, sW0, t + 1);
    }
    if (t < full) {
        step(sA0, sW0, sA1, sW1, t);
        for (int h = 0; h < tail; ++h) part(sA1, sW1, h);
    } else {
        for (int h = 0; h < tail; ++h) part(sA0, sW0, h);
    }
    // epilogue (k_gemm's EPI_BIAS_ACT): C/D layout col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int col = n0 + wave * 32 + (lane & 31);
    if (col < N) {
        const float bj = bias ? bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (row < M) {
                float v = acc[r];
                v += bj;
                if (act == AZD_ACT_RELU) v = v > 0.f ? v : 0.f;
                else if (act == AZD_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
                const size_t orow = rows_out ? (size_t)rows_out[row] : (size_t)row;
                Y[orow * (size_t)ldy + col] = v;
            }
        }
    }
}

static void launch_gemm_f32_gathered(hipStream_t st, const float *A, int lda, const float *W, int ldw, float *Y, int ldy, int max_rows, int N, int K,
                                     int act, const float *bias, const uint32_t *m_dev, const uint32_t *rows_in, const uint32_t *rows_out) {
    const bool vec = K % 4 == 0 && lda % 4 == 0 && ldw % 4 == 0 && ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(W)) & 15) == 0;
    const unsigned blocks = (unsigned)(((max_rows + GF_BM - 1) / GF_BM) * ((N + GF_BN - 1) / GF_BN));
    if (vec) k_gemm_f32_gathered<true><<<dim3(blocks), dim3(256), 0, st>>>(A, lda, W, ldw, Y, ldy, max_rows, N, K, act, bias, m_dev, rows_in, rows_out);
    else k_gemm_f32_gathered<false><<<dim3(blocks), dim3(256), 0, st>>>(A, lda, W, ldw, Y, ldy, max_rows, N, K, act, bias, m_dev, rows_in, rows_out);
}

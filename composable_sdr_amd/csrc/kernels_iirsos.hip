// iirCFilter / iirFilterN / iirFilterSOS (csdr_iirsos_*): a cascade of S second-order sections with real
// coefficients on nchan independent rows of F32 or CF32 samples.
//   k_iirsos<CPLX> : one workgroup per row, built on k_biquad's blocked scan (kernels_wbfm.hip).  Per section, direct form II:
//                      v0 = x - a1 v1 - a2 v2 ;  y = b0 v0 + b1 v1 + b2 v2
//                    which is linear in the state s = (v1, v2): s' = A s + B x.  The row is walked in chunks of 4096 samples.
//                    A chunk is loaded into LDS once (16 bytes per lane where the rows allow it, the next chunk's loads in
//                    flight while this one is computed), then every section runs over it in place, one after the other: a
//                    thread runs its 16 consecutive samples from zero state, a Hillis-Steele scan over the 256 thread end states
//                    in f64 with that section's own powers A^(16 2^k) yields every thread's true start state, a second pass
//                    writes the section's outputs over its inputs.  Then the chunk is stored once: a sample crosses HBM twice
//                    whatever S is.  A thread reads and writes only its own 16 LDS slots between the load and the store, so
//                    the sections need no barrier of their own beyond the scan's.  Complex rows carry (re, im) through the same
//                    scan with the same real matrices.  Every section's state crosses chunks and calls exactly; only the f32
//                    summation order differs from the sequential loop.  A first-order section is one with a2 = b2 = 0.
//                    No workgroup waits for another: a row is one workgroup's work, so nchan = 1 runs on one CU.
#include "../../include/csdr.h"
#include "csdr_internal.h"

namespace csdr {

namespace {

constexpr int IS_T = 256, IS_PER = 16, IS_CHUNK = IS_T * IS_PER;

template <bool CPLX> struct IsTypes;
template <> struct IsTypes<false> { using T = float; using St = float2; static constexpr int NC = 1; };
template <> struct IsTypes<true> { using T = float2; using St = float4; static constexpr int NC = 2; };

__device__ __forceinline__ float is_zero(float) { return 0.f; }
__device__ __forceinline__ float2 is_zero(float2) { return make_float2(0.f, 0.f); }
// a v + acc, a (v) alone
__device__ __forceinline__ float is_fma(float a, float v, float acc) { return fmaf(a, v, acc); }
__device__ __forceinline__ float2 is_fma(float a, float2 v, float2 acc) { return make_float2(fmaf(a, v.x, acc.x), fmaf(a, v.y, acc.y)); }
__device__ __forceinline__ float is_mul(float a, float v) { return a * v; }
__device__ __forceinline__ float2 is_mul(float a, float2 v) { return make_float2(a * v.x, a * v.y); }
__device__ __forceinline__ float is_comp(float v, int) { return v; }
__device__ __forceinline__ float is_comp(float2 v, int j) { return j ? v.y : v.x; }
__device__ __forceinline__ void is_make(float &v, const double *d) { v = (float)d[0]; }
__device__ __forceinline__ void is_make(float2 &v, const double *d) { v = make_float2((float)d[0], (float)d[1]); }
__device__ __forceinline__ float2 is_state(float v1, float v2) { return make_float2(v1, v2); }
__device__ __forceinline__ float4 is_state(float2 v1, float2 v2) { return make_float4(v1.x, v1.y, v2.x, v2.y); }
__device__ __forceinline__ void is_unstate(float2 s, float &v1, float &v2) { v1 = s.x; v2 = s.y; }
__device__ __forceinline__ void is_unstate(float4 s, float2 &v1, float2 &v2) { v1 = make_float2(s.x, s.y); v2 = make_float2(s.z, s.w); }

// LDS slot of sample s of the chunk: thread s / 16 owns 16 consecutive slots, padded to 17 (k_biquad's layout)
__device__ __forceinline__ uint32_t is_slot(uint32_t s) { return 17u * (s >> 4) + (s & 15u); }

// X, Y [C][n] of T (the same array or disjoint ones, hence no __restrict__); sec [S]; st [C][S] section states (v1, v2), read at
// the start and written where the row ends
template <bool CPLX>
__global__ __launch_bounds__(IS_T) void k_iirsos(const void *Xv, void *Yv, uint32_t n, uint32_t S,
                                                 const IirSosSection *__restrict__ sec, void *__restrict__ stv, uint32_t vec)
{
    using T = typename IsTypes<CPLX>::T;
    using St = typename IsTypes<CPLX>::St;
    constexpr int NC = IsTypes<CPLX>::NC;             // real components per sample
    constexpr int PV = 16 / sizeof(T);                // samples per 16-byte access
    constexpr int NV = IS_PER / PV;                   // 16-byte accesses per thread and chunk
    __shared__ T xs[17 * IS_T];
    __shared__ double sc[2][2 * NC][IS_T];            // scan ping-pong: v1 (re, im), v2 (re, im), one array per component
    __shared__ St carry_s[IIRSOS_MAX_SEC];
    const int tid = threadIdx.x;
    const uint32_t c = blockIdx.x;
    const T *row = static_cast<const T *>(Xv) + (size_t)c * n;
    T *orow = static_cast<T *>(Yv) + (size_t)c * n;
    St *st = static_cast<St *>(stv) + (size_t)c * S;
    if (tid < (int)S) carry_s[tid] = st[tid];

    // the chunk at `base` into registers: whole 16-byte accesses where the launch allows it (vec: every row starts on a 16-byte
    // boundary and holds a whole number of them), single samples otherwise; zeros behind the row's end
    float4 pre[NV];
    auto fetch = [&](uint32_t base) {
        if (vec) {
#pragma unroll
            for (int i = 0; i < NV; i++) {
                const uint32_t t = base + PV * (tid + IS_T * i);
                pre[i] = t < n ? *reinterpret_cast<const float4 *>(row + t) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {
            T *p = reinterpret_cast<T *>(pre);
#pragma unroll
            for (int i = 0; i < IS_PER; i++) {
                const uint32_t t = base + tid + IS_T * i;
                p[i] = t < n ? row[t] : is_zero(T());
            }
        }
    };
    fetch(0);
    for (uint32_t base = 0; base < n; base += IS_CHUNK) {
        if (vec) {
#pragma unroll
            for (int i = 0; i < NV; i++) {
                const uint32_t s = PV * (tid + IS_T * i);
                const T *p = reinterpret_cast<const T *>(&pre[i]);
#pragma unroll
                for (int j = 0; j < PV; j++) xs[is_slot(s) + j] = p[j];      // s is a multiple of PV: the PV slots are adjacent
            }
        } else {
            const T *p = reinterpret_cast<const T *>(pre);
#pragma unroll
            for (int i = 0; i < IS_PER; i++) xs[is_slot(tid + IS_T * i)] = p[i];
        }
        __syncthreads();                               // also orders carry_s (the loads above, the last chunk's writes)
        if (base + IS_CHUNK < n) fetch(base + IS_CHUNK);                     // in flight during the sections below
        T x[IS_PER];
#pragma unroll
        for (int k = 0; k < IS_PER; k++) x[k] = xs[17 * tid + k];
        for (uint32_t q = 0; q < S; q++) {
            const IirSosSection &p = sec[q];
            const float b0 = p.b0, k1 = p.k1, k2 = p.k2, na1 = -p.a1, na2 = -p.a2;   // y = b0 x + k1 v1 + k2 v2 (pre-state)
            T c1, c2;
            is_unstate(carry_s[q], c1, c2);
            // pass 1: end state from zero state (thread 0: from the carried state, so that its end state is the true one)
            T v1 = tid == 0 ? c1 : is_zero(T()), v2 = tid == 0 ? c2 : is_zero(T());
#pragma unroll
            for (int k = 0; k < IS_PER; k++) {
                const T v0 = is_fma(na2, v2, is_fma(na1, v1, x[k]));
                v2 = v1; v1 = v0;
            }
            // inclusive scan of s_i = A^16 s_{i-1} + e_i over the threads, in f64 (k_biquad: a narrow low-pass keeps a state
            // thousands of times larger than its output, and A^n has entries ~n for poles near the unit circle).  The buffer a
            // section starts in alternates: the last section's results are still being read from the other one
            double sv[2 * NC];
#pragma unroll
            for (int j = 0; j < NC; j++) { sv[j] = (double)is_comp(v1, j); sv[NC + j] = (double)is_comp(v2, j); }
            int cur = q & 1;
#pragma unroll
            for (int j = 0; j < 2 * NC; j++) sc[cur][j][tid] = sv[j];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int d = 1 << k;
                if (tid >= d) {
                    const double p0 = p.pw[k][0], p1 = p.pw[k][1], p2 = p.pw[k][2], p3 = p.pw[k][3];
#pragma unroll
                    for (int j = 0; j < NC; j++) {
                        const double u1 = sc[cur][j][tid - d], u2 = sc[cur][NC + j][tid - d];
                        sv[j] = fma(p0, u1, fma(p1, u2, sv[j]));
                        sv[NC + j] = fma(p2, u1, fma(p3, u2, sv[NC + j]));
                    }
                }
#pragma unroll
                for (int j = 0; j < 2 * NC; j++) sc[cur ^ 1][j][tid] = sv[j];
                cur ^= 1;
                __syncthreads();
            }
            // pass 2 from the true start state; the outputs replace the inputs, in registers and (last section) in LDS
            if (tid) {
                double u[2 * NC];
#pragma unroll
                for (int j = 0; j < 2 * NC; j++) u[j] = sc[cur][j][tid - 1];
                is_make(v1, u); is_make(v2, u + NC);
            } else { v1 = c1; v2 = c2; }
#pragma unroll
            for (int k = 0; k < IS_PER; k++) {
                const T y = is_fma(b0, x[k], is_fma(k1, v1, is_mul(k2, v2)));
                const T v0 = is_fma(na2, v2, is_fma(na1, v1, x[k]));
                v2 = v1; v1 = v0;
                x[k] = y;
                // the row may end inside this chunk: the state after its last sample is what the next call needs
                if (base + (uint32_t)(IS_PER * tid + k) == n - 1) st[q] = is_state(v1, v2);
            }
            if (tid == IS_T - 1) carry_s[q] = is_state(v1, v2);
        }
#pragma unroll
        for (int k = 0; k < IS_PER; k++) xs[17 * tid + k] = x[k];
        __syncthreads();
        if (vec) {
#pragma unroll
            for (int i = 0; i < NV; i++) {
                const uint32_t s = PV * (tid + IS_T * i), t = base + s;
                float4 o;
                T *p = reinterpret_cast<T *>(&o);
#pragma unroll
                for (int j = 0; j < PV; j++) p[j] = xs[is_slot(s) + j];
                if (t < n) *reinterpret_cast<float4 *>(orow + t) = o;
            }
        } else {
#pragma unroll
            for (int i = 0; i < IS_PER; i++) {
                const uint32_t s = tid + IS_T * i, t = base + s;
                if (t < n) orow[t] = xs[is_slot(s)];
            }
        }
        __syncthreads();                               // xs is free for the next chunk
    }
}

}  // namespace

int launch_iirsos(bool cplx, const void *x, void *y, uint32_t C, uint32_t n, uint32_t S, const IirSosSection *sec, void *state,
                  hipStream_t s)
{
    if (!C || !n) return 0;
    const size_t el = cplx ? sizeof(float2) : sizeof(float);
    const uint32_t vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0 && ((size_t)n * el) % 16 == 0;
    if (cplx) hipLaunchKernelGGL(k_iirsos<true>, dim3(C), dim3(IS_T), 0, s, x, y, n, S, sec, state, vec);
    else hipLaunchKernelGGL(k_iirsos<false>, dim3(C), dim3(IS_T), 0, s, x, y, n, S, sec, state, vec);
    CSDR_HIP(hipGetLastError());
    return 0;
}

}  // namespace csdr

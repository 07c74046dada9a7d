// Single-pass fused channelizer kernel for gfx950 (wave64, 256 CUs, 160 KiB LDS/CU), M = 256.
//
//   raw CF32 x  --DC blocker--> y --14-tap polyphase FIR + NCO pre-mix--> X_t[j]
//               --256-point forward DFT (16 x 16)--> Y_t[k] --transpose--> channel-major
//               --per-channel freqdem--> out[C][nf]          (8 B read + 4/8 B written per sample)
//
// One workgroup (256 threads) produces one TILE of 16 frames (4096 input samples) and never
// writes an intermediate to HBM.  The stream-long recurrences are cut at tile boundaries:
//   * DC blocker (iirfilt_crcf, v[n] = x[n] + beta v[n-1], y = x - alpha v[n-1]) is a linear
//     scan.  Each tile's zero-state aggregate A_b is published as two 8-byte {tag,value}
//     granules as soon as the tile has been read; a tile's carry is the decayed sum of the
//     previous ten aggregates (beta^40960 = 1.3e-9 truncation) -- a decoupled look-back that
//     never chains, because an aggregate does not depend on any other workgroup.
//   * The FIR needs the 13 frames before the tile: the workgroup re-reads the previous tile
//     (an L2 hit: its owner is reading it at the same time) and re-runs the DC blocker on it.
//   * freqdem needs the previous frame's channel sample: each tile publishes its last Y
//     frame (2 KiB) and the successor picks it up in its tail phase.
// Workgroups take their tile index from an atomic ticket, so every tile a workgroup waits on
// belongs to a workgroup that has already started and publishes before it waits (no deadlock
// under any dispatch order; inter-workgroup data uses agent-scope atomics only).
//
// Thread roles inside a tile (tid = 0..255):
//   stage    thread q = run of 16 consecutive samples: serial DC scan, 16-lane DPP row scan
//   FIR      thread j = polyphase branch j           : window of 13 + 16 frames in VGPRs
//   pass 1   thread (f, b)  : Z_f[k1][b] = W256^(b k1) sum_a X_f[16a+b] W16^(a k1)
//   pass 2   thread (f, k1) : Y_f[k1+16 k2] = sum_b Z_f[k1][b] W16^(b k2)
//   tail     thread k       : 16 consecutive time samples of channel k
// MFMA is not used: the path is streaming FIR/FFT bounded by HBM and VALU (north_star).
//
// Replaces per chunk: iirfilt_crcf_execute_block + nco_crcf_mix_block_down + nf x
// firpfbch_crcf_analyzer_execute + the Haskell transpose (Liquid.chs:575-589, 828-862) and
// M x freqdem_demodulate_block (Liquid.chs:324-328).
#include "fused_common.h"
#include <cstring>

namespace csdr {

namespace {

#define STAMP(i) do { if (A.trace && tid == 0) A.trace[(size_t)b * 16 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)

template <bool FM>
__global__ __launch_bounds__(256) void k_tile256(TileArgs A)
{
    __shared__ __attribute__((aligned(16))) float2 R[LDS_F2];
    __shared__ float2 tw_s[M256];
    __shared__ float2 Tt[2][16];        // frame totals: [0] own, [1] halo
    __shared__ float2 carry_s[2];       // c_b, c_{b-1}
    __shared__ unsigned tile_s;

    const int tid = threadIdx.x;
    if (tid == 0) tile_s = atomicAdd(A.ticket, 1u);
    tw_s[tid] = A.tw[tid];
    __syncthreads();
    const unsigned b = tile_s;
    if (b >= A.nb) return;
    STAMP(0);   // ticket known
    const int nvalid = (int)min(16u, A.nf - 16u * b);
    const int j = tid;
    const int col_off = 16 * (j >> 4) + 2 * (((j & 15) >> 1) ^ (j >> 5)) + (j & 1);
    float2 *E = R + E_OFF;

    // ---------------- issue the global loads: own tile and the tile before it ----------------
    float4 raw_o[8], raw_h[8];
    tile_load(reinterpret_cast<const float4 *>(A.x) + (size_t)b * 2048, 16 * nvalid, raw_o, tid);
    if (b > 0) tile_load(reinterpret_cast<const float4 *>(A.x) + (size_t)(b - 1) * 2048, 256, raw_h, tid);

    // ---------------- own tile: stage, scan, publish the aggregate ----------------
    stage_and_scan(raw_o, R, E, Tt[0], A, tid);
    STAMP(1);   // own tile loaded + scanned

    float2 nw[NB], old[NB];
#pragma unroll
    for (int f = 0; f < NB; f++) { nw[f] = R[256 * f + col_off]; old[f] = make_float2(0.f, 0.f); }

    if (tid < 64) {
        // zero-state frame chain of the own tile -> aggregate A_b, published as two granules
        if (tid == 0) {
            float2 v = make_float2(0.f, 0.f);
#pragma unroll
            for (int f = 0; f < 16; f++) v = cfma(v, A.b256[1], Tt[0][f]);
            __hip_atomic_store(&A.agg[2 * (size_t)b], ((u64)A.epoch << 32) | __float_as_uint(v.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.agg[2 * (size_t)b + 1], ((u64)A.epoch << 32) | __float_as_uint(v.y), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // ---------------- look-back: carries c_b (own tile) and c_{b-1} (halo tile) ----------------
        const int lane = tid;
        float2 cb = make_float2(0.f, 0.f), cp = make_float2(0.f, 0.f);
        const int k = lane;                                  // lane k in 1..LOOKBACK looks at tile b-k
        const bool need = (k >= 1 && k <= LOOKBACK && (int)b - k >= 0);
        u64 g0 = 0, g1 = 0;
        unsigned spins = 0;
        bool ok = !need;
        while (true) {
            if (need && !ok) {
                g0 = __hip_atomic_load(&A.agg[2 * (size_t)(b - k)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                g1 = __hip_atomic_load(&A.agg[2 * (size_t)(b - k) + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = (unsigned)(g0 >> 32) == A.epoch && (unsigned)(g1 >> 32) == A.epoch;
            }
            if (__all(ok)) break;
            if (++spins > SPIN_LIMIT) { if (lane == 0) atomicOr(A.status, 1u); break; }
            __builtin_amdgcn_s_sleep(2);
        }
        if (need) {
            const float2 Ak = make_float2(__uint_as_float((unsigned)g0), __uint_as_float((unsigned)g1));
            cb = make_float2(Ak.x * A.wtile[k - 1], Ak.y * A.wtile[k - 1]);
            if (k >= 2) cp = make_float2(Ak.x * A.wtile[k - 2], Ak.y * A.wtile[k - 2]);
        }
        if (lane == 0) {                                     // the stream state before this call
            const float2 ve = A.vend_in[0];
            if (b <= LOOKBACK) cb = make_float2(ve.x * A.wtile[b], ve.y * A.wtile[b]);
            if (b >= 1 && b - 1 <= LOOKBACK) cp = make_float2(ve.x * A.wtile[b - 1], ve.y * A.wtile[b - 1]);
        }
        // sum over lanes 0..15 (one DPP row): the inclusive row_shr ladder ends in lane 15
        cb = cadd(cb, dpp2<0x111>(cb)); cp = cadd(cp, dpp2<0x111>(cp));
        cb = cadd(cb, dpp2<0x112>(cb)); cp = cadd(cp, dpp2<0x112>(cp));
        cb = cadd(cb, dpp2<0x114>(cb)); cp = cadd(cp, dpp2<0x114>(cp));
        cb = cadd(cb, dpp2<0x118>(cb)); cp = cadd(cp, dpp2<0x118>(cp));
        if (lane == 15) { carry_s[0] = cb; carry_s[1] = cp; }
    }
    STAMP(2);   // look-back done (wave 0)
    __syncthreads();                                            // own z consumed; carries ready
    STAMP(3);

    // ---------------- halo: the 13 frames before the tile ----------------
    if (b > 0) {
        stage_and_scan(raw_h, R, E + 256, Tt[1], A, tid);
#pragma unroll
        for (int f = 3; f < NB; f++) old[f] = R[256 * f + col_off];
    } else {
#pragma unroll
        for (int f = 3; f < NB; f++) old[f] = A.yhist_in[(f - 3) * M256 + j];
    }

    STAMP(4);   // halo staged + scanned
    // ---------------- carry into every run: P[q] = beta^(16 r) * (v before frame f) + E[q] ----------------
    {
        const int fq = tid >> 4;
        const float br = A.b16[tid & 15], bf = A.b256[fq];
        const float2 v0 = cfma(carry_s[0], bf, frame_carry_zero_state(Tt[0], A, tid));
        E[tid] = cfma(v0, br, E[tid]);
        if (b > 0) {
            const float2 v1 = cfma(carry_s[1], bf, frame_carry_zero_state(Tt[1], A, tid));
            E[256 + tid] = cfma(v1, br, E[256 + tid]);
        }
        if (b == A.nb - 1 && tid == 16 * ((nvalid - 1) & 15) + 15) {
            // DC blocker state after the last valid frame: v before it, advanced over that frame
            // (the thread owning the frame's last run: v0 is v before frame nvalid-1)
            A.vend_out[0] = cfma(v0, A.b256[1], Tt[0][nvalid - 1]);
        }
    }
    __syncthreads();

    // ---------------- finish the DC blocker: y = z - alpha*beta^i * P[run] ----------------
    {
        const float kj = -A.alpha * A.bj[j & 15];
#pragma unroll
        for (int f = 0; f < NB; f++) nw[f] = cfma(E[16 * f + (j >> 4)], kj, nw[f]);
        if (b > 0) {
#pragma unroll
            for (int f = 3; f < NB; f++) old[f] = cfma(E[256 + 16 * f + (j >> 4)], kj, old[f]);
        }
    }
    if (b == A.nb - 1) {
        // stream state for the next call: DC v1 after the last frame, the last 13 frames of y
        const int base = (int)A.nf - 13 - 16 * (int)b;        // tile-relative frame of yhist slot 0
#pragma unroll
        for (int f = 3; f < NB; f++) {
            const int d = (f - 16) - base;
            if (d >= 0 && d < 13) A.yhist_out[d * M256 + j] = old[f];
        }
#pragma unroll
        for (int f = 0; f < NB; f++) {
            const int d = f - base;
            if (d >= 0 && d < 13 && f < nvalid) A.yhist_out[d * M256 + j] = nw[f];
        }
    }
    __syncthreads();                                            // P consumed, R free
    STAMP(5);   // DC blocker finished

    // ---------------- polyphase FIR + NCO pre-mix ----------------
    // u[t][j] = y[t][j] * wpre[parity(t)][j] and X_t[j] = sum_n h[(255-j)+256n] u[t-n][j]:
    // even and odd taps see the two phasors, so two partial sums and two complex products.
    {
        float h[P];
#pragma unroll
        for (int n = 0; n < P; n++) h[n] = A.taps[(M256 - 1 - j) + n * M256];
        const float2 Wa = A.wpre[(A.parity0 & 1) * M256 + j], Wb = A.wpre[((A.parity0 & 1) ^ 1) * M256 + j];
        const v2f Wav = to_v(Wa), Wbv = to_v(Wb);
#pragma unroll
        for (int f = 0; f < NB; f += 2) {
            // complex x real multiply-accumulate as one packed f32 FMA per tap; two frames at a time so that
            // consecutive FMAs are independent
            v2f ev[2] = {{0.f, 0.f}, {0.f, 0.f}}, od[2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
            for (int n = P - 1; n >= 0; n--) {
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const int i = f + q - n;
                    const float2 s2 = (i >= 0) ? nw[i] : old[NB + i];
                    const v2f sv = {s2.x, s2.y}, hv = {h[n], h[n]};
                    if (n & 1) od[q] = __builtin_elementwise_fma(sv, hv, od[q]); else ev[q] = __builtin_elementwise_fma(sv, hv, ev[q]);
                }
            }
            // frame f is even within the tile: its even taps see Wa, its odd taps Wb; frame f+1 the other way
            cmul2_v(ev[0], Wav, od[0], Wbv);
            cmul2_v(ev[1], Wbv, od[1], Wav);
            R[f * FS_X + j] = to_f2(ev[0] + od[0]);
            R[(f + 1) * FS_X + j] = to_f2(ev[1] + od[1]);
        }
    }
    __syncthreads();                                            // X complete
    STAMP(6);   // FIR done

    // ---------------- DFT pass 1: thread (f, b1) ----------------
        v2f vv[16];
        {
            const int f = tid >> 4, b1 = tid & 15;
#pragma unroll
            for (int a = 0; a < 16; a++) vv[a] = to_v(R[f * FS_X + 16 * a + b1]);
            fft16_v(vv);
#pragma unroll
            for (int i = 1; i < 16; i++) vv[i] = cmul_v(vv[i], to_v(tw_s[16 * XIDX(i) + b1]));
            __syncthreads();                                        // everyone has read X
#pragma unroll
            for (int i = 0; i < 16; i++) R[f * FS_Z + XIDX(i) * RS_Z + b1] = to_f2(vv[i]);
        }
        __syncthreads();                                            // Z complete
    STAMP(7);   // pass 1 done

    // ---------------- DFT pass 2: thread (f, k1) ----------------
        {
            const int f = tid >> 4, k1 = tid & 15;
#pragma unroll
            for (int b1 = 0; b1 < 16; b1++) vv[b1] = to_v(R[f * FS_Z + k1 * RS_Z + b1]);
            fft16_v(vv);
            __syncthreads();                                        // everyone has read Z
#pragma unroll
            for (int i = 0; i < 16; i++) R[(k1 + 16 * XIDX(i)) * RS_Y + f] = to_f2(vv[i]);
        }
        __syncthreads();                                            // Y complete
    STAMP(8);   // pass 2 done

    // ---------------- tail: thread k owns channel k ----------------
    float2 v[16];
#pragma unroll
    for (int f = 0; f < NB; f++) v[f] = R[tid * RS_Y + f];
    const bool owned = (uint32_t)tid >= A.c0 && (uint32_t)tid < A.c0 + A.C;
    const size_t row = (size_t)(owned ? tid - A.c0 : 0) * A.out_stride + A.out_t0 + (size_t)16 * b;

    if (FM) {
        // publish my last valid frame for the next tile, then fetch the previous tile's
        float2 last = v[0];
#pragma unroll
        for (int f = 1; f < NB; f++) if (f < nvalid) last = v[f];
        const u64 bits = ((u64)__float_as_uint(last.y) << 32) | __float_as_uint(last.x);
        __hip_atomic_store(&A.ylast[(size_t)b * M256 + tid], bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(&A.yflag[b], A.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (b == A.nb - 1 && owned) A.rp_out[tid - A.c0] = last;
        STAMP(9);   // last frame published

        float m[NB];
        if (owned) {
#pragma unroll
            for (int f = 1; f < NB; f++) {
                const float2 rp = v[f - 1], r = v[f];
                // arg(conj(r') r): products rounded separately like the reference's C expression
                const float re = __fadd_rn(__fmul_rn(rp.x, r.x), __fmul_rn(rp.y, r.y));
                const float im = __fsub_rn(__fmul_rn(rp.x, r.y), __fmul_rn(rp.y, r.x));
                m[f] = fast_atan2f(im, re) * A.fm_ref;
            }
        }
        float2 prev;
        if (b == 0) {
            prev = owned ? A.rp_in[tid - A.c0] : make_float2(0.f, 0.f);
        } else {
            unsigned spins = 0;
            while (__hip_atomic_load(&A.yflag[b - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != A.epoch) {
                if (++spins > SPIN_LIMIT) { if (tid == 0) atomicOr(A.status, 2u); break; }
                __builtin_amdgcn_s_sleep(2);
            }
            const u64 pb = __hip_atomic_load(&A.ylast[(size_t)(b - 1) * M256 + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            prev = make_float2(__uint_as_float((unsigned)pb), __uint_as_float((unsigned)(pb >> 32)));
        }
        STAMP(10);  // previous tile's last frame received
        if (owned) {
            {
                const float2 r = v[0];
                const float re = __fadd_rn(__fmul_rn(prev.x, r.x), __fmul_rn(prev.y, r.y));
                const float im = __fsub_rn(__fmul_rn(prev.x, r.y), __fmul_rn(prev.y, r.x));
                m[0] = fast_atan2f(im, re) * A.fm_ref;
            }
            float *o = (float *)A.out + row;
            if (((A.out_stride | A.out_t0) % 4u) == 0 && nvalid == NB) {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    *reinterpret_cast<float4 *>(o + 4 * q) = make_float4(m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]);
            } else {
#pragma unroll
                for (int f = 0; f < NB; f++) if (f < nvalid) o[f] = m[f];
            }
        }
    } else if (owned) {
        float2 *o = (float2 *)A.out + row;
        if (((A.out_stride | A.out_t0) % 2u) == 0 && nvalid == NB) {
#pragma unroll
            for (int q = 0; q < 8; q++)
                *reinterpret_cast<float4 *>(o + 2 * q) = make_float4(v[2 * q].x, v[2 * q].y, v[2 * q + 1].x, v[2 * q + 1].y);
        } else {
#pragma unroll
            for (int f = 0; f < NB; f++) if (f < nvalid) o[f] = v[f];
        }
    }
    STAMP(11);  // stores issued
}


}  // namespace

// (make_split -- nb tiles into nruns runs, whole tile pairs with the same total on every CU: run_split.h)

// The chunk's last WU + 1 raw tiles -> the plan's tail slot (a kernel on the launch's own stream rather than a D2D memcpy: no
// copy engine, no blit-path synchronisation in front of the run kernel)
__global__ __launch_bounds__(256) void k_save_tail(const float4 *__restrict__ src, float4 *__restrict__ dst)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    dst[i] = src[i];
}

// ragged end of an interleaved shard's call: rows c0 + G m of the whole-band tile result [256][rem] -> the shard's plane [C][nf] at frame t0
// (w = floats per sample: 1 F32, 2 CF32)
__global__ __launch_bounds__(64) void k_shard_gather(const float *__restrict__ src, float *__restrict__ dst, uint32_t c0, uint32_t G, uint32_t rem,
                                                     uint32_t nf, uint32_t t0, uint32_t w)
{
    const uint32_t m = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < rem * w; i += 64) dst[((size_t)m * nf + t0) * w + i] = src[(size_t)(c0 + G * m) * rem * w + i];
}

// k_run256v2: the older of a CU's two workgroups wins the issue arbitration and runs ~1.4x faster than the younger one, so it gets the
// larger share of the tiles (measured: both end together at about 1.2 : 0.8); rotating the priority per tile instead was no better
constexpr float V2_WEIGHT_CF[8] = {1.2f, 0.8f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
constexpr float V2_WEIGHT_FM[8] = {1.24f, 0.76f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};      // with whole-line stores the younger workgroup loses more (r03 trace: 4.8 vs 7.6 us per tile)
// whole-band FM (one tile buffer, three workgroups per CU): shares of the oldest, the middle and the youngest workgroup of a CU
// (make_split turns the shares into whole tile pairs per run, the same on every CU: 16 + 10 + 6 pairs at the bench size.  Measured on exact
// triples, profiles/r08_run_split_ab.txt: (16, 10, 6) ahead of (15, 10, 7), (17, 9, 6), (16, 9, 7), (15, 11, 6), (17, 10, 5), (16, 11, 5), (14, 11, 7), (14, 12, 6))
constexpr float V2_WEIGHT_FM3[8] = {1.6f, 1.f, 0.6f, 1.f, 1.f, 1.f, 1.f, 1.f};
constexpr float EQUAL_WEIGHT[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};

struct FusedPlan : ChainPlan {
    using ChainPlan::ChainPlan;
    enum { K_TILE256 = 0, K_RUN256V2 };      // KernelChoice::id
    uint32_t max_nb = 0, epoch = 0;
    float *d_taps = nullptr;
    float2 *d_tw = nullptr, *d_wpre = nullptr;
    StreamState st;
    unsigned *d_ticket = nullptr, *d_yflag = nullptr, *d_status = nullptr;
    u64 *d_agg = nullptr, *d_ylast = nullptr;
    // whole-band run-kernel launches without warm-up windows (RunArgs::nowu, round 5): DC state in front of every run's halo tile, the
    // uncorrected near-DC channels of every run's first tiles, the chain's response to a unit DC state (k_run256_dcfix)
    ColdStart cold;
    u64 *d_trace = nullptr;
    uint32_t run_min_tiles = 1024;   // chunks with at least this many tiles use the run kernel (measured crossover: FM ~900 tiles, CF32 ~700; profiles/r04_call_size_sweeps.txt)
    float slot_weight[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};   // CSDR_RUN_WEIGHTS: tile share of the k-th co-resident run of a CU
    uint32_t slot_pairs[8] = {0, 0, 0, 0, 0, 0, 0, 0};                 // CSDR_RUN_PAIRS: its tile pairs, given outright
    bool have_weights = false, have_pairs = false;
    bool pd_equal = false, pd_nocopy = false;     // CSDR_PD_EQUAL, CSDR_PD_NOCOPY: scheduling experiments of the independent launches (the second: wrong run-0 starts)
    uint32_t resident_wgs_v2 = 512;  // workgroups of k_run256v2 the device holds at once
    // independent launches (csdr_chain_submit_device): the last WU + 1 raw tiles of the previous chunk, three slots (the launch
    // two calls back may still be reading its slot when this call's copy is queued on the other stream)
    float *d_shard_tail = nullptr;   // interleaved shard: whole-band result of a call's ragged end, [256][< 16] CF32 at most
    float4 *d_tail[3] = {nullptr, nullptr, nullptr};
    int tail_w = 0;                  // slot that holds the tail of the most recent chunk
    bool tail_valid = false, save_tails = false;
    TileArgs proto;                  // what init() fixes of a k_tile256 launch
    RunArgs run_proto;               // and of a k_run256v2 launch: the DC and phase constants, the cold-start arrays and the launch knobs

    int init();
    KernelChoice choose(uint32_t nf) const override;
    const char *kernel_name(int id) const override;
    // until the first call csdr_chain_path names the tile kernel, whatever a call of max_nf frames would take (the route strings are read by tools and logs)
    KernelChoice first_choice() const override { return {K_TILE256, 0}; }
    bool tile_major_ok(uint32_t nf) const override;
    void keep_tail() override { save_tails = cfg.G == 1; }     // interleaved shards never run as independent launches
    bool can_overlap(uint32_t nf) const override;
    bool tail_recorded() const override { return save_tails && tail_valid; }
    int status(unsigned *st) override;
    int trace(unsigned long long *out, uint32_t ntiles) override;
    int reset_state(hipStream_t s) override;
    int run(const FusedCall &call, KernelChoice k, void *out, hipStream_t s, KernelTimer *timer) override;
    void wire_state(TileArgs &A) const;
    int run_kernel(const FusedCall &call, const TileArgs &A, uint32_t nruns, hipStream_t s, KernelTimer *timer);
    int tile_kernel(TileArgs &T, hipStream_t s, KernelTimer *timer);
    int ragged_end(const FusedCall &call, void *out, uint32_t nb_full, uint32_t rem, hipStream_t s);
};

bool plan256_supported(uint32_t M, uint32_t p) { return M == 256 && p == P; }
int plan256_create(const FusedConfig &cfg, ChainPlan **out) { return make_plan<FusedPlan>(cfg, out); }

// a comma-separated knob into at most eight values
template <class T, class Conv> static void parse_list(const char *e, T (&v)[8], Conv conv)
{
    int k = 0;
    for (const char *q = e; *q && k < 8; k++) { v[k] = (T)conv(q); q = strchr(q, ','); if (!q) break; q++; }
}

int FusedPlan::init()
{
    int r;
    max_nb = (cfg.max_nf + NB - 1) / NB;
    if ((r = mem.alloc(&d_taps, sizeof(float) * cfg.M * cfg.p))) return r;
    if ((r = mem.alloc(&d_tw, sizeof(float2) * cfg.M))) return r;
    if ((r = mem.alloc(&d_wpre, sizeof(float2) * 2 * cfg.M))) return r;
    if ((r = st.alloc(mem, 13 * cfg.M, cfg.G > 1 ? cfg.M : cfg.C))) return r;     // interleaved shard: full-band indices (fused_v2: rp_in / rp_out)
    if (cfg.G > 1 && (r = mem.alloc(&d_shard_tail, sizeof(float2) * cfg.M * NB))) return r;
    for (int i = 0; i < 3; i++) {
        if ((r = mem.alloc(&d_tail[i], sizeof(float4) * 2048 * (WU + 1)))) return r;
        CSDR_HIP(hipMemset(d_tail[i], 0, sizeof(float4) * 2048 * (WU + 1)));
    }
    tail_valid = true;               // a fresh stream: zero history IS the exact history
    if ((r = mem.alloc(&d_ticket, sizeof(unsigned)))) return r;
    if ((r = mem.alloc(&d_status, sizeof(unsigned)))) return r;
    if ((r = mem.alloc(&d_yflag, sizeof(unsigned) * max_nb))) return r;
    if ((r = mem.alloc(&d_agg, sizeof(u64) * 2 * max_nb))) return r;
    if ((r = mem.alloc(&d_ylast, sizeof(u64) * (size_t)cfg.M * max_nb))) return r;
    if (const char *e = diag_env("CSDR_RUN_MIN_TILES")) run_min_tiles = (uint32_t)atol(e);
    if (cfg.mix && (r = mem.alloc(&d_premix, (size_t)cfg.C * cfg.max_nf * (cfg.fm ? 4 : 8)))) return r;
    const char *trace_knob = diag_env("CSDR_TRACE");
    if (trace_knob) {
        if ((r = mem.alloc(&d_trace, sizeof(u64) * 16 * max_nb))) return r;
        CSDR_HIP(hipMemset(d_trace, 0, sizeof(u64) * 16 * max_nb));
    }
    CSDR_HIP(hipMemcpy(d_taps, cfg.taps, sizeof(float) * cfg.M * cfg.p, hipMemcpyHostToDevice));
    std::vector<float2> tw(cfg.M);
    for (uint32_t k1 = 0; k1 < 16; k1++)
        for (uint32_t b1 = 0; b1 < 16; b1++) {
            const double a = -2.0 * 3.14159265358979323846 * (double)(b1 * k1) / (double)cfg.M;
            tw[16 * k1 + b1] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
    const std::vector<float2> wpre = premix_table();
    CSDR_HIP(hipMemcpy(d_tw, tw.data(), sizeof(float2) * cfg.M, hipMemcpyHostToDevice));
    CSDR_HIP(hipMemcpy(d_wpre, wpre.data(), sizeof(float2) * 2 * cfg.M, hipMemcpyHostToDevice));
    // Whole band: the response of the chain, at the channels 126..129, to a DC-blocker state of 1 in front of a tile.  Frames 15 .. 127
    // behind the tile's start = frame -1 .. 111 of the run that started its halo tile without its state (k_run256_dcfix: 112 frames); by
    // then the step's edge (13 frames of FIR, every channel) has left the filter and what remains sits around DC.
    if (cfg.G == 1 && cfg.c0 == 0 && cfg.C == cfg.M &&
        (r = cold.init(mem, cfg, (DCFIX_F - 1) * 256.0, RUN256_COLD_RUNS, (size_t)4 * DCFIX_F, false, 15u, (uint32_t)DCFIX_F, 126, wpre.data()))) return r;
    CSDR_HIP(hipMemset(d_status, 0, sizeof(unsigned)));
    CSDR_HIP(hipMemset(d_yflag, 0, sizeof(unsigned) * max_nb));
    CSDR_HIP(hipMemset(d_agg, 0, sizeof(u64) * 2 * max_nb));

    TileArgs &A = proto;
    A = TileArgs{};
    A.taps = d_taps; A.tw = d_tw; A.wpre = d_wpre;
    A.ticket = d_ticket; A.agg = d_agg; A.ylast = d_ylast; A.yflag = d_yflag; A.status = d_status;
    A.c0 = cfg.c0; A.C = cfg.C; A.fm_ref = cfg.fm_ref; A.trace = d_trace;
    dcc.put(A);
    if (const char *e = diag_env("CSDR_CUS")) { if (atoi(e) > 0 && (uint32_t)atoi(e) < cus) cus = (uint32_t)atoi(e); }     // experiments: a plan sized for a CU-masked stream
    resident_wgs_v2 = (uint32_t)(cus * run256_v2_blocks_per_cu(cfg.fm, cfg.G));
    if (const char *e = diag_env("CSDR_RESIDENT_WGS")) resident_wgs_v2 = (uint32_t)atol(e);
    if (const char *e = diag_env("CSDR_RUN_WEIGHTS")) { parse_list(e, slot_weight, atof); have_weights = true; }
    // tile pairs per run of each class, e.g. 15,11,6 (make_split ignores it unless it sums to the pairs of a CU)
    if (const char *e = diag_env("CSDR_RUN_PAIRS")) { parse_list(e, slot_pairs, atol); have_pairs = true; }
    pd_equal = diag_env("CSDR_PD_EQUAL") != nullptr;
    pd_nocopy = diag_env("CSDR_PD_NOCOPY") != nullptr;

    RunArgs &RA = run_proto;
    RA = RunArgs{};
    RA.pk = phase_consts(cfg.fm_ref);
    RA.l2beta = dcc.l2beta;
    RA.cpre = cold.cpre; RA.side = cold.side;
    { const char *e = diag_env("CSDR_PRIO_ROT"); RA.prio_div = (e && atoi(e)) ? cus : 0u; }
    RA.trace_light = (trace_knob && atoi(trace_knob) == 2) ? 1u : 0u;
    { const char *e = diag_env("CSDR_WU"); RA.wu = e ? (uint32_t)atoi(e) : (uint32_t)WU; }       // experiments: fewer tiles = wrong DC state at run starts
    { const char *e = diag_env("CSDR_WU_ROT"); RA.wu_rot = e ? (uint32_t)atoi(e) : 0u; }      // measured: no effect on the run-start burst
    RA.pair_align = (cfg.fm || diag_env("CSDR_PAIR_ALIGN_CF")) ? 1u : 0u;
    { const char *e = diag_env("CSDR_WU_BATCH6"); RA.wu_batch6 = e ? (uint32_t)atoi(e) : 1u; }
    return 0;
}

int FusedPlan::reset_state(hipStream_t s)
{
    if (int r = st.reset(s)) return r;
    CSDR_HIP(hipMemsetAsync(d_tail[0], 0, sizeof(float4) * 2048 * (WU + 1), s));
    tail_w = 0; tail_valid = true;
    return 0;
}

// k_run256v2 takes the whole tiles of every call of an interleaved shard (the tile kernel only knows whole bands) and the whole-band calls of
// >= run_min_tiles tiles; a contiguous channel shard takes the tile kernel, which masks its stores, at every size
KernelChoice FusedPlan::choose(uint32_t nf) const
{
    const uint32_t nb = nf / NB;
    if (cfg.G == 1 && !(cfg.c0 == 0 && cfg.C == cfg.M && nb >= run_min_tiles)) return {K_TILE256, 0};
    // one run per resident workgroup slot (a single round), runs balanced to within one tile,
    // at least 8 tiles per run so that the warm-up reads stay below 7/8 of a run
    const uint32_t nruns = resident_wgs_v2 < nb / 8 ? resident_wgs_v2 : nb / 8;
    return {K_RUN256V2, nruns ? nruns : 1};
}

const char *FusedPlan::kernel_name(int id) const
{
    static const char *const run[2][4] = {{"k_run256v2<CF32>", "k_run256v2<CF32>/G2", "k_run256v2<CF32>/G4", "k_run256v2<CF32>/G8"},
                                          {"k_run256v2<FM>", "k_run256v2<FM>/G2", "k_run256v2<FM>/G4", "k_run256v2<FM>/G8"}};
    if (id == K_RUN256V2) return run[cfg.fm][cfg.G == 8 ? 3 : cfg.G == 4 ? 2 : cfg.G == 2 ? 1 : 0];
    return cfg.fm ? "k_tile256<FM>" : "k_tile256<CF32>";
}

bool FusedPlan::tile_major_ok(uint32_t nf) const
{
    // the calls that go to k_run256v2 as whole tiles: CF32 output below 4 GiB, no mix inside the plan
    if (cfg.fm || cfg.mix || nf % NB || !nf || (cfg.G > 1 && (uint64_t)cfg.C * nf * 8u >= (1ull << 32))) return false;
    return choose(nf).id == K_RUN256V2;
}

bool FusedPlan::can_overlap(uint32_t nf) const
{
    return save_tails && tail_valid && nf % NB == 0 && !cfg.mix && choose(nf).id == K_RUN256V2;     // (save_tails: whole band)
}

void FusedPlan::wire_state(TileArgs &A) const
{
    A.yhist_in = st.hist_in(cur); A.yhist_out = st.hist_out(cur);
    A.vend_in = st.vend_in(cur);  A.vend_out = st.vend_out(cur);
    A.rp_in = st.rp_in(cur);      A.rp_out = st.rp_out(cur);
}

int FusedPlan::run(const FusedCall &call, KernelChoice k, void *out, hipStream_t s, KernelTimer *timer)
{
    const FusedConfig &c = cfg;
    const uint32_t nf = call.nf, nb_full = nf / NB, rem = nf - nb_full * NB;
    const bool shard = c.G > 1;      // interleaved shard: every whole tile goes through k_run256v2<.., G> (the tile kernel only knows whole bands)
    if (shard && (uint64_t)c.C * nf * (c.fm ? 4u : 8u) >= (1ull << 32)) { set_error("fused: interleaved shard output of %u frames exceeds 4 GiB", nf); return -1; }
    int r;
    TileArgs A = proto;
    A.x = call.d_in;
    A.out = out;
    wire_state(A);
    A.out_stride = call.tile_major ? NB : nf;      // tile-major: a row's 16 frames of a tile are one 128-byte line; rows follow each other inside the tile's block
    A.out_t0 = 0;
    A.parity0 = (uint32_t)(frames_done & 1);
    if (k.id == K_RUN256V2) {
        // large chunk: dependency-free runs of full tiles (k_run256v2; its lane offsets are 32-bit over 16 rows and the row groups
        // go through a 64-bit base, so the output may exceed 4 GiB); a ragged tail (< 16 frames) follows as a second launch of the
        // tile kernel on the state the run kernel leaves behind
        A.nf = nb_full * NB; A.nb = nb_full;
        if ((r = run_kernel(call, A, k.runs, s, timer))) return r;
        if (rem && (r = ragged_end(call, out, nb_full, rem, s))) return r;
    } else {
        tail_valid = false;
        A.nf = nf; A.nb = (nf + NB - 1) / NB;
        if ((r = tile_kernel(A, s, timer))) return r;
    }
    CSDR_HIP(hipGetLastError());
    return 0;
}

// The whole tiles of a call (A.nb of them; none: a shard's call of fewer than 16 frames, which ragged_end does alone) through k_run256v2
int FusedPlan::run_kernel(const FusedCall &call, const TileArgs &A, uint32_t nruns, hipStream_t s, KernelTimer *timer)
{
    const FusedConfig &c = cfg;
    const bool shard = c.G > 1;
    int r;
    RunArgs RA = run_proto;
    RA.t = A;
    RA.nruns = nruns;
    const float *v2_weight = c.fm ? ((cus && nruns == 3 * cus) ? V2_WEIGHT_FM3 : V2_WEIGHT_FM) : V2_WEIGHT_CF;
    RA.split = make_split(A.nb, nruns, cus, (call.indep && pd_equal) ? EQUAL_WEIGHT : (have_weights ? slot_weight : v2_weight),
                          have_pairs ? slot_pairs : nullptr);
    RA.tile_step = call.tile_major ? c.C * 128u : (uint32_t)NB * (c.fm ? 4u : 8u);
    RA.indep = call.indep ? 1u : 0u;     // (process() has checked can_overlap)
    // whole band, dependent launches: no warm-up windows (the DC state a run misses at its start is put back, where it still matters 16 frames
    // later -- the four channels around DC -- by k_run256_dcfix behind the launch); runs of >= 8 tiles, as many as the arrays are made for
    RA.nowu = (cold.fits(nruns) && run256_v2_cold(nruns) && !shard && !RA.indep) ? 1u : 0u;
    RA.prev_tail = d_tail[tail_w];
    if (save_tails && !shard && call.nf == A.nb * NB && A.nb >= WU + 1) {
        // this chunk's last WU + 1 tiles, for run 0 of the next call (queued in front of the launch: the copy only reads the input)
        const int nxt = (tail_w + 1) % 3;
        if (!pd_nocopy) hipLaunchKernelGGL(k_save_tail, dim3(2048 * (WU + 1) / 256), dim3(256), 0, s,
                                           reinterpret_cast<const float4 *>(call.d_in + (size_t)(A.nb - (WU + 1)) * 4096), d_tail[nxt]);
        if (call.ev_tail) CSDR_HIP(hipEventRecord(call.ev_tail, s));
        tail_w = nxt; tail_valid = true;
    } else tail_valid = false;
    if (timer && (r = timer->begin(s))) return r;
    if (A.nb && (r = run256_v2_launch(&RA, c.fm, c.G, nruns, s))) return r;
    if (RA.nowu && A.nb && (r = run256_dcfix_launch(&RA, c.fm, nruns, cold.rt, s))) return r;
    if (timer && (r = timer->end(s))) return r;             // the bracket covers k_run256_dcfix: it is part of every no-warm-up step
    return 0;
}

// One k_tile256 launch of T.nb tiles: a new epoch for the look-back tags, the ticket counter back to zero
int FusedPlan::tile_kernel(TileArgs &T, hipStream_t s, KernelTimer *timer)
{
    int r;
    if (++epoch == 0) epoch = 1;
    T.epoch = epoch;
    CSDR_HIP(hipMemsetAsync(d_ticket, 0, sizeof(unsigned), s));
    if (timer && (r = timer->begin(s))) return r;
    if (cfg.fm) hipLaunchKernelGGL(k_tile256<true>, dim3(T.nb), dim3(256), 0, s, T);
    else hipLaunchKernelGGL(k_tile256<false>, dim3(T.nb), dim3(256), 0, s, T);
    if (timer && (r = timer->end(s))) return r;
    return 0;
}

// The rem < 16 frames behind a run-kernel call's nb_full whole tiles: one tile of k_tile256 on the state the run kernel leaves behind
int FusedPlan::ragged_end(const FusedCall &call, void *out, uint32_t nb_full, uint32_t rem, hipStream_t s)
{
    const FusedConfig &c = cfg;
    const bool shard = c.G > 1;
    int r;
    if (nb_full) cur ^= 1;                            // the tail starts from the run kernel's state
    TileArgs T = proto;
    T.x = call.d_in + (size_t)nb_full * NB * c.M; T.out = out;
    wire_state(T);
    T.nf = rem; T.nb = 1; T.out_stride = call.nf; T.out_t0 = nb_full * NB;
    if (shard) { T.c0 = 0; T.C = c.M; T.out = d_shard_tail; T.out_stride = rem; T.out_t0 = 0; }   // whole band into [256][rem], the owned rows are gathered below
    T.parity0 = (uint32_t)((frames_done + nb_full * NB) & 1);
    if ((r = tile_kernel(T, s, nullptr))) return r;
    if (shard) hipLaunchKernelGGL(k_shard_gather, dim3(c.C), dim3(64), 0, s, (const float *)d_shard_tail, (float *)out, c.c0, c.G, rem,
                                  call.nf, nb_full * NB, c.fm ? 1u : 2u);
    return 0;
}


int FusedPlan::trace(unsigned long long *out, uint32_t ntiles)
{
    (void)hipDeviceSynchronize();
    if (!d_trace) return 0;
    if (ntiles > max_nb) ntiles = max_nb;
    CSDR_HIP(hipMemcpy(out, d_trace, sizeof(u64) * 16 * ntiles, hipMemcpyDeviceToHost));
    return (int)ntiles;
}

int FusedPlan::status(unsigned *st)
{
    CSDR_HIP(hipMemcpy(st, d_status, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (*st) CSDR_HIP(hipMemset(d_status, 0, sizeof(unsigned)));     // sticky until reported once
    return 0;
}

}  // namespace csdr

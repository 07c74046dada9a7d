// firpfbch2Synthesizer (the synthesizer side of liquid's firpfbch2_crcf, which the reference does not import): the
// way back from the rows of the 2x-oversampled channelizer of kernels_pfb2.hip to one stream.  M channels (a power of two,
// 4 .. 256), a real prototype g[0 .. L - 1], L = 2 m M, P = M / 2; every frame of M values Y[k][t] gives P output samples.
//   k_pfb2s<2 m, log2 M> : 512 threads; a workgroup walks a run of consecutive tiles of F = 4096 / M frames (pfb2_shape.h)
//                          load + DFT + FIR + store in one launch, nothing in between goes through HBM
// LDS of a workgroup (pfb2s_lds_bytes): the accumulator carry [L - P] | V [F][row stride] | the twiddles [M / 4] | the taps [L].
// A tile: F consecutive frames of every row are read in whole 128-byte pieces (lanes along the frames) into V, row k at slot
// bitrev(k) of its frame; the DFT runs in place in V, radix-2 decimation in time, two stages per pass (one single stage first when
// log2 M is odd), so that slot q ends as w_t[q] in natural order with no reorder pass: the mirror of k_pfb2's decimation in frequency.
// The FIR is the transpose of k_pfb2's: a linear accumulator window of L - P + F P output samples, sample s of it owned by thread
// s mod 512 for the whole run (F P = 2048 is a multiple of 512, so the owner does not change when the window moves on).  The owner
// adds the tile's frames u in ascending order, acc = fma(g[s - u P], w_u[s_abs mod M], acc): no atomics, no order between threads,
// and lanes on consecutive s read consecutive slots of V.  Behind a tile the window's first F P sums are final: they leave from the
// register they were summed in, times 0.5, as one contiguous store (the run's ends masked).  The other L - P partial sums go to the
// carry, F P slots further down, which only their owner reads again: the window's move costs no pass and no barrier, and only
// the carry needs LDS.  The taps are an LDS copy, read by consecutive lanes at consecutive addresses: a tile holds F of the 4 m
// frames that reach a sample, so the taps a sample meets in a tile are a range [n_lo, n_hi] that differs from sample to sample, and
// a loop over that range cannot index registers (4 m predicated steps over register taps cost 64 VGPRs as packed operands, spilled
// from m = 6 on, and waited for every LDS read inside a branch).  Without the window's F P slots the copy fits: two workgroups per CU
// at every (M, m).
// A run starts from +0 and walks the 4 m - 1 frames in front of its first output frame first, from the call or, in front of the
// call's first frame, from the handle's history of input frames; what they add to samples in front of the run is dropped.  That
// halo makes the runs independent of each other.  The next tile's frames are fetched into registers ahead of the FIR.
// Arithmetic contract: f32, no contraction beyond the fmas named here.  w_t = the unscaled backward DFT of frame t: butterflies
// a + c w, a - c w with w = e^{+2 pi j p / N} from pfb2_twiddles (M / 4 entries; the second quarter is j times the first), a complex
// product is g_cmul of fft16_generic.h; the order of operations depends on M only.  With s = t P + r, r < P:
// acc = +0; for n = 4 m - 1 down to 0 with t - n >= 0 (frames in front of the stream are skipped, not taken as zero):
// acc = fma(g[r + n P], w_{t-n}[(r + t P) mod M], acc), re and im packed; x[s] = 0.5 acc, exact.  t counts frames from the start of
// the stream (the handle carries its parity and how many frames it has seen, up to 4 m - 1).  Nothing depends on where a frame
// falls in a tile, a run or a call: the output is bit-identical for every chunking.
#include "../../include/csdr.h"
#include "csdr_internal.h"
#include "fft16_generic.h"

#pragma clang fp contract(off)

namespace csdr {

namespace {

constexpr int P2S_T = PFB2_THREADS;
constexpr int P2S_ITEMS = 4096 / P2S_T;     // (frame, row) items of a tile per thread: F M = 4096

typedef v2fg c32;                            // one CF32 value in a register pair: the adds, products and fmas below are packed
__device__ __forceinline__ c32 mulj(c32 a) { return (c32){-a.y, a.x}; }

// row k of frame f of the call (f < 0: the history, whose last frame is frame -1 and which holds `seen` frames of the stream);
// frames in front of the stream and frames from `end` on read as zero and are never added
__device__ __forceinline__ c32 frame_at(const c32 *__restrict__ y, const c32 *__restrict__ hist, uint32_t k, int f, uint32_t frames,
                                        int end, int HF, int seen)
{
    if (f >= end || f < -seen) return (c32){0.f, 0.f};
    return f >= 0 ? y[(size_t)k * frames + (uint32_t)f] : hist[(int)k * HF + HF + f];
}

template <int TM, int LOGM>
__global__ __launch_bounds__(P2S_T, 4) void k_pfb2s(const float2 *__restrict__ y_, float2 *__restrict__ x_, const float *__restrict__ g,
                                                     const float2 *__restrict__ tw_, const float2 *__restrict__ hist_in_,
                                                     float2 *__restrict__ hist_out_, Pfb2sLaunch l)
{
    const c32 *__restrict__ y = reinterpret_cast<const c32 *>(y_), *__restrict__ tw = reinterpret_cast<const c32 *>(tw_);
    const c32 *__restrict__ hist_in = reinterpret_cast<const c32 *>(hist_in_);
    c32 *__restrict__ x = reinterpret_cast<c32 *>(x_), *__restrict__ hist_out = reinterpret_cast<c32 *>(hist_out_);
    extern __shared__ float4 lds4[];
    constexpr uint32_t M = 1u << LOGM, P = M >> 1, LOGP = LOGM - 1, L = TM * M, CARRY = L - P, LOGF = 12 - LOGM, F = 1u << LOGF, FP = F * P;
    constexpr uint32_t VS = pfb2_row_stride(M), Q = M >> 2, W = CARRY + FP;
    constexpr int NT = 2 * TM, HF = NT - 1;                  // taps of a phase; frames in front of a sample's own that reach it
    constexpr int NS = (W + P2S_T - 1) / P2S_T, QSTEP = P2S_T >> LOGP;
    static_assert(F == pfb2_tile_frames(M) && CARRY == pfb2s_carry_slots(M, TM / 2) && HF == (int)pfb2s_halo_frames(TM / 2) &&
                  FP % P2S_T == 0 && P2S_T % P == 0 && F * M == P2S_ITEMS * P2S_T && F * Q == 2 * P2S_T, "pfb2_shape.h");
    const uint32_t tid = threadIdx.x, frames = l.frames;
    const int seen = (int)l.seen;
    c32 *A = reinterpret_cast<c32 *>(lds4);
    c32 *V = A + CARRY;
    c32 *twl = V + F * VS;
    float *gl = reinterpret_cast<float *>(twl + Q);

    for (uint32_t k = tid; k < Q; k += P2S_T) twl[k] = tw[k];
    for (uint32_t k = tid; k < L; k += P2S_T) gl[k] = g[k];
    // the stream's next history: the last 4 m - 1 frames of (history | call), row-major [M][4 m - 1]; the call is not empty
    if (blockIdx.x == 0) {
        for (uint32_t e = tid; e < M * HF; e += P2S_T) {
            const uint32_t k = e / HF;
            const int j = (int)(e - k * HF);
            hist_out[e] = frame_at(y, hist_in, k, (int)frames - HF + j, frames, (int)frames, HF, seen);
        }
    }
    const uint32_t tile0 = blockIdx.x * l.tiles_per_run;
    const uint32_t tile1 = min(tile0 + l.tiles_per_run, l.tiles);
    const int f0 = (int)(tile0 * F), f1 = (int)min(tile1 * F, frames);   // the run's output frames
    const int64_t s_lo = (int64_t)f0 * P, s_hi = (int64_t)f1 * P;
    for (uint32_t k = tid; k < CARRY; k += P2S_T) A[k] = (c32){0.f, 0.f};
    const uint32_t r = tid & (P - 1);
    const int q0 = (int)(tid >> LOGP);
    // the run's first tile of input frames starts 4 m - 1 frames in front of its first output frame
    int fb = f0 - HF;
#pragma unroll
    for (int i = 0; i < P2S_ITEMS; i++) {
        const uint32_t e = tid + P2S_T * i, fl = e & (F - 1), gr = e >> LOGF;
        // 16 frames per row piece: the two rows of a half-wave are k and k + M / 2, one slot apart in V
        const uint32_t k = F >= 32 ? gr : ((gr & 1u) << (LOGM - 1)) | (gr >> 1);
        V[fl * VS + (__brev(k) >> (32 - LOGM))] = frame_at(y, hist_in, k, fb + (int)fl, frames, f1, HF, seen);
    }
    __syncthreads();

    for (; fb < f1; fb += (int)F) {
        const int nf = min((int)F, f1 - fb);
        const bool more = fb + (int)F < f1;
        // backward DFT of every frame, in place, bit-reversed in, natural out: block length N, two stages per pass
        if (LOGM & 1) {
#pragma unroll
            for (int i = 0; i < (int)((F * P) / P2S_T); i++) {
                const uint32_t e = tid + P2S_T * i, fl = e & (F - 1), b = e >> LOGF;
                c32 *v = V + fl * VS + 2 * b;
                const c32 a = v[0], c = v[1];
                v[0] = a + c; v[1] = a - c;
            }
            __syncthreads();
        }
#pragma unroll
        for (int logN = (LOGM & 1) ? 3 : 2; logN <= LOGM; logN += 2) {
            const uint32_t N = 1u << logN, q = N >> 2, logq = logN - 2, sh = LOGM - logN;
#pragma unroll 1
            for (int i = 0; i < 2; i++) {
                const uint32_t e = tid + P2S_T * i;          // lanes run over the frames: the row stride keeps them on different banks
                const uint32_t fl = e & (F - 1), b = e >> LOGF, pos = b & (q - 1), blk = b >> logq;
                c32 *v = V + fl * VS + blk * N + pos;
                const c32 a0 = v[0], a1 = v[q], a2 = v[2 * q], a3 = v[3 * q];
                const uint32_t i2 = (2 * pos) << sh;
                const c32 wa = twl[pos << sh], w1 = i2 < Q ? twl[i2] : mulj(twl[i2 - Q]);
                const c32 t1 = g_cmul(a1, w1), t3 = g_cmul(a3, w1);                  // stage N / 2: pairs q apart
                const c32 b0 = a0 + t1, b1 = a0 - t1, b2 = a2 + t3, b3 = a2 - t3;
                const c32 u2 = g_cmul(b2, wa), u3 = mulj(g_cmul(b3, wa));            // stage N: pairs 2 q apart, the second with j wa
                v[0] = b0 + u2; v[2 * q] = b0 - u2;
                v[q] = b1 + u3; v[3 * q] = b1 - u3;
            }
            __syncthreads();
        }
        // the next tile's frames, into registers
        c32 pre[P2S_ITEMS];
        if (more) {
#pragma unroll
            for (int i = 0; i < P2S_ITEMS; i++) {
                const uint32_t e = tid + P2S_T * i, fl = e & (F - 1), gr = e >> LOGF;
                const uint32_t k = F >= 32 ? gr : ((gr & 1u) << (LOGM - 1)) | (gr >> 1);
                pre[i] = frame_at(y, hist_in, k, fb + (int)F + (int)fl, frames, f1, HF, seen);
            }
        }
        // FIR: window slot e is sample fb P + e of the call, phase r = e mod P, frame fb + q with q = e / P.  The tile's frame ul
        // meets it with tap n = q - ul; the slot of w it reads, (r + (t0 + fb + q) P) mod M, is the same for all of them
        const int ulo = max(0, -seen - fb);                  // the tile's first frame that belongs to the stream
        const uint32_t parb = (l.par0 + (uint32_t)fb) & 1u;
#pragma unroll 1
        for (int j = 0; j < NS; j++) {
            const uint32_t e = tid + P2S_T * j;
            if (e < W) {
                const int q = q0 + QSTEP * j;
                const c32 *vp = V + (r + ((((uint32_t)q + parb) & 1u) << LOGP));
                c32 acc = {0.f, 0.f};
                if (e < CARRY) acc = A[e];
                // the taps whose frame q - n is one of the tile's and of the stream's, oldest frame first
                const int nlo = max(0, q - (nf - 1)), nhi = min(NT - 1, q - ulo);
                const c32 *vq = vp + q * (int)VS;
#pragma unroll 4
                for (int n = nhi; n >= nlo; n--) {
                    const float gn = gl[r + n * (int)P];
                    acc = __builtin_elementwise_fma((c32){gn, gn}, vq[-n * (int)VS], acc);
                }
                if (e < FP) {
                    const int64_t s = (int64_t)fb * P + e;
                    if (s >= s_lo && s < s_hi) x[s] = acc * 0.5f;
                } else {
                    A[e - FP] = acc;
                }
            }
        }
        __syncthreads();
        if (more) {
#pragma unroll
            for (int i = 0; i < P2S_ITEMS; i++) {
                const uint32_t e = tid + P2S_T * i, fl = e & (F - 1), gr = e >> LOGF;
                const uint32_t k = F >= 32 ? gr : ((gr & 1u) << (LOGM - 1)) | (gr >> 1);
                V[fl * VS + (__brev(k) >> (32 - LOGM))] = pre[i];
            }
            __syncthreads();
        }
    }
}

using LaunchFn = hipError_t (*)(dim3, size_t, hipStream_t, const float2 *, float2 *, const float *, const float2 *, const float2 *, float2 *,
                                const Pfb2sLaunch &);
template <int TM, int LOGM>
hipError_t launch_one(dim3 grid, size_t lds, hipStream_t s, const float2 *y, float2 *x, const float *g, const float2 *tw,
                      const float2 *hist_in, float2 *hist_out, const Pfb2sLaunch &l)
{
    if (lds > 64 * 1024) {           // per device, so asked for at every such launch
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pfb2s<TM, LOGM>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)PFB2_LDS_LIMIT);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_pfb2s<TM, LOGM>), grid, dim3(P2S_T), lds, s, y, x, g, tw, hist_in, hist_out, l);
    return hipGetLastError();
}
template <int LOGM> LaunchFn by_semi(uint32_t m)
{
    switch (m) {
    case 1: return launch_one<2, LOGM>;   case 2: return launch_one<4, LOGM>;   case 3: return launch_one<6, LOGM>;
    case 4: return launch_one<8, LOGM>;   case 5: return launch_one<10, LOGM>;  case 6: return launch_one<12, LOGM>;
    case 7: return launch_one<14, LOGM>;  case 8: return launch_one<16, LOGM>;
    }
    return nullptr;
}
LaunchFn by_shape(uint32_t M, uint32_t m)
{
    switch (M) {
    case 4: return by_semi<2>(m);    case 8: return by_semi<3>(m);    case 16: return by_semi<4>(m);   case 32: return by_semi<5>(m);
    case 64: return by_semi<6>(m);   case 128: return by_semi<7>(m);  case 256: return by_semi<8>(m);
    }
    return nullptr;
}

}  // namespace

int launch_pfb2s(const float2 *y, float2 *x, const float *g, const float2 *tw, const float2 *hist_in, float2 *hist_out, uint32_t M,
                 uint32_t m, uint32_t frames, uint32_t parity, uint32_t seen, uint32_t cus, hipStream_t s)
{
    if (!frames) return 0;
    if (!pfb2_args_ok(M, m) || seen > pfb2s_halo_frames(m)) {
        set_error("pfbsyn2: M = %u, m = %u, %u frames of history are not a launch shape", M, m, seen);
        return CSDR_ERR_INVALID;
    }
    const Pfb2Shape sh = pfb2s_shape(M, m, frames, cus);
    if (sh.lds > PFB2_LDS_LIMIT) {
        set_error("pfbsyn2: M = %u, m = %u need %zu bytes of LDS (limit %zu)", M, m, sh.lds, PFB2_LDS_LIMIT);
        return CSDR_ERR_SIZE;
    }
    const LaunchFn launch = by_shape(M, m);
    if (!launch) { set_error("pfbsyn2: no kernel for M = %u, m = %u", M, m); return CSDR_ERR_INVALID; }
    Pfb2sLaunch l;
    l.frames = frames; l.par0 = parity & 1u; l.seen = seen; l.tiles = sh.tiles; l.tiles_per_run = sh.tiles_per_run;
    CSDR_HIP(launch(dim3(sh.runs), sh.lds, s, y, x, g, tw, hist_in, hist_out, l));
    return 0;
}

}  // namespace csdr

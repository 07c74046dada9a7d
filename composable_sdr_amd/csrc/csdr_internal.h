// Internal declarations shared by the HIP translation units of libcsdr_hip.so.
// Product code: must not include or link anything under oracle/.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "agc_tail_shape.h"
#include "pfb2_shape.h"
#include "rowresamp_shape.h"
#include "psktrack_common.h"

namespace csdr {

// ---- error plumbing -------------------------------------------------------
void set_error(const char *fmt, ...);
int  hip_fail(hipError_t e, const char *what, const char *file, int line);
#define CSDR_HIP(call)                                                          \
    do {                                                                        \
        hipError_t e__ = (call);                                                \
        if (e__ != hipSuccess) return ::csdr::hip_fail(e__, #call, __FILE__, __LINE__); \
    } while (0)

// ---- device buffers released together (fused plans, chain and block handles) ---------
// alloc() records every buffer it makes; the destructor frees them all
struct DeviceBuffers {
    DeviceBuffers() = default;
    DeviceBuffers(const DeviceBuffers &) = delete;
    DeviceBuffers &operator=(const DeviceBuffers &) = delete;
    ~DeviceBuffers() { for (void *q : owned) (void)hipFree(q); }
    template <class T> int alloc(T **p, size_t bytes) {      // hipMalloc of `bytes` (at least one) into *p
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes ? bytes : 1);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc", __FILE__, __LINE__);
        owned.push_back(q);
        *p = static_cast<T *>(q);
        return 0;
    }
    template <class T> int alloc_n(T **p, size_t n) { return alloc(p, sizeof(T) * (n ? n : 1)); }   // n elements (at least one)
private:
    std::vector<void *> owned;
};

// ---- diagnostics knobs ------------------------------------------------------
// The CSDR_* variables that change a launch plan (CSDR_RUN_MIN_TILES, CSDR_RUN_WEIGHTS, CSDR_AGC_L / _W, CSDR_WU, CSDR_RUN1024_V3, ...:
// DESIGN.md section 6.1; several of them change RESULTS) exist for A/B measurements and for the tests that force a kernel onto a small
// input.  They are read only when CSDR_DIAG=1 is set next to them: a production host does not inherit a knob from its environment by
// accident.  (Read when a handle is created or a plan is made, never inside a launch loop.)  Not gated: CSDR_QUIET (a print),
// CSDR_RCCL_LIB (where librccl lives), CSDR_LIB (which build of this library the Python binding loads).
inline const char *diag_env(const char *name)
{
    const char *d = getenv("CSDR_DIAG");
    return (d && d[0] == '1' && d[1] == 0) ? getenv(name) : nullptr;
}

// ---- host-side design (design.cpp) -----------------------------------------
// Kaiser prototype of firpfbch_crcf_create_kaiser(ANALYZER, M, m, As)
// (reference call: Liquid.chs:813).  Returns the M*2m taps the bank uses.
std::vector<float> design_pfb_taps(uint32_t M, uint32_t m, float As);
// msresamp_crcf(r, As) decomposition and filters (reference call: Liquid.chs:104, rate = bw/fs, As = 60)
struct ResampDesign {
    float rate = 0.f; double rho = 0.0; uint32_t K = 0;
    std::vector<uint32_t> m_hb; std::vector<std::vector<float>> h_hb;   // half-band stage s: 4 m + 1 taps
    uint32_t npfb = 256, m_arb = 7; float fc = 0.f; std::vector<float> pfb;   // [npfb][2 m_arb]
    uint64_t delta = 0;          // input samples per output at the arbitrary stage, Q32.32
};
ResampDesign design_msresamp(float rate, float As);
// nco_crcf_set_frequency's float -> uint32 phase-step conversion.
uint32_t nco_freq_word(float freq);
// Haskell-Float value of  -0.5*(M-1)/M*2*pi  (Liquid.chs:817).
float pfb_premix_freq(uint32_t M);
// cos/sin of one uint32 phase, evaluated like nco_crcf (VCO) does.
void nco_phasor(uint32_t theta, float *c, float *s);
// Period (in samples) of the phase sequence k*d_theta mod 2^32; 0 if > limit.
uint32_t nco_period(uint32_t d_theta, uint32_t limit);
// Smallest gain g for which rssi(g) = (float)(-20*log10(g)) is NOT above thr:
// squelch "threshold exceeded"  <=>  g < returned value.
float agc_gain_threshold(float threshold_db);

// ---- device-side parameter blocks ------------------------------------------
constexpr int DC_THREADS = 256;
constexpr int DC_PER_THREAD = 8;
constexpr int DC_BLOCK = DC_THREADS * DC_PER_THREAD;   // samples per scan block

struct DcParams {
    float a1;              // -(1-alpha)        (v0 = x - a1*v1)
    float beta;            // 1-alpha as f32 = -a1
    float beta_pow_thr[9]; // beta^(DC_PER_THREAD * 2^i), i=0..8
    double beta_blk;       // beta^DC_BLOCK (f64)
    float log2_beta;
};

// DC shortcuts: a route that cuts the DC blocker's state after a window of N samples (read-only warm-up tiles, look-back
// tiles, the dcfix corrections behind cold starts) was sized for the default alpha = 0.0005.  It may serve a handle whose beta^N is no
// larger than what the same window leaves at that alpha (for every N this amounts to alpha >= 0.0005), and whose warm-up folds can
// form their weight ratio beta^-512 in f32 (alpha below ~0.15; above it the fold's 0 * inf is NaN).  A handle that fails takes the
// any-M route with the exact block scan (launch_dc_mix).
inline bool dc_window_ok(const DcParams &dc, double N)
{
    const double b = dc.beta, b0 = (double)(1.0f - 0.0005f);
    return b > 0.0 && __builtin_pow(b, N) <= __builtin_pow(b0, N) && -512.0 * __builtin_log2(b) < 120.0;
}

struct NcoParams {
    uint32_t theta0;       // phase of the first sample of this call
    uint32_t d_theta;
    uint32_t tab_len;      // 0: evaluate sincos on device; else period of the table
    uint32_t tab_pos;      // index of the first sample of this call in the table
    int      up;           // 1: multiply by v, 0: by conj(v)
};

struct AgcParams {
    float alpha;           // 0.1
    float g_thr;           // exceeded <=> g < g_thr
    uint32_t timeout;      // 1000
};

// per-channel AGC state as kept on the device between chunks
struct AgcState { float g, y2; int32_t mode; uint32_t timer; };

// ---- generic kernels (kernels_generic.hip) ----------------------------------
// DC blocker [+ NCO mix] of n samples: y[i] = mix(dcblock(x[i])).  `state` is the
// device-resident v1 (float2), updated in place.  scratch: >= 2*ceil(n/DC_BLOCK)+2 float2.
int launch_dc_mix(const float2 *x, float2 *y, uint32_t n, bool do_dc, const DcParams &dc,
                  float2 *state, float2 *scratch, bool do_mix, const NcoParams &nco,
                  const float2 *nco_tab, hipStream_t s);
// X[t][j] = sum_n h[(M-1-j)+n*M] * u[(t-n)*M + j], u points at the first NEW sample and
// has (p-1)*M samples of history in front of it.
int launch_pfb_fir(const float2 *u, const float *taps, float2 *X, uint32_t M, uint32_t p,
                   uint32_t nf, hipStream_t s);
// forward M-point DFT of every frame: Y[t][k].  tw: e^{-j 2 pi i/M}, i<M.
int launch_dft(const float2 *X, float2 *Y, const float2 *tw, uint32_t M, uint32_t nf, hipStream_t s);
// interleaved channel shard g of G: Z[t][j1] = W_M^{j1 g} sum_{j2 < G} X[t][j1 + (M/G) j2] W_G^{j2 g}; the (M/G)-point DFT of Z[t]
// is Y[t][g + G m].  ph: G phasors W_G^{j2 g} followed by M/G phasors W_M^{j1 g}
int launch_fold(const float2 *X, float2 *Z, const float2 *ph, uint32_t M, uint32_t G, uint32_t nf, hipStream_t s);
// out[t] = sum_k DFT(X[t])[k] in k_mix_frames' summation order, without materialising Y (M = 1024, 4096, all channels)
bool dft_mix_supported(uint32_t M);
int launch_dft_mix(const float2 *X, float2 *out, const float2 *tw, uint32_t M, uint32_t nf, hipStream_t s);
// fused FIR + DFT + transpose [+ freqdem] for M = 1024 (kernels_pfb1024.hip): u_new as for launch_pfb_fir; out = channel-major
// [C][nf] CF32, or F32 with fm; scratch: 2 * min(max_runs, nf/32) * 1024 float2
bool pfb1024_supported(uint32_t M, uint32_t p);
int launch_pfb1024(const float2 *u_new, const float *taps, const float2 *tw, void *out, bool fm, uint32_t nf, uint32_t c0, uint32_t C,
                   float ref, const float2 *rp_in, float2 *rp_out, float2 *scratch, uint32_t max_runs, hipStream_t s);
// Z[c][t] = Y[t][c0 + c]  for c < C
int launch_transpose(const float2 *Y, float2 *Z, uint32_t M, uint32_t nf, uint32_t c0, uint32_t C,
                     hipStream_t s);
// per-channel AGC + squelch mute, in place on Z[C][nf]
int launch_agc(float2 *Z, uint32_t C, uint32_t nf, AgcState *st, const AgcParams &p, hipStream_t s);
// F[c][t] = arg(conj(prev)*Z[c][t]) * ref ; rp_in/rp_out: per-channel r'
int launch_fm(const float2 *Z, float *F, uint32_t C, uint32_t nf, float ref, const float2 *rp_in,
              float2 *rp_out, hipStream_t s);
// out[i] = ((in[0][i] + in[1][i]) + ...) + in[C-1][i], row length E floats
int launch_mix(const float *in, float *out, uint32_t C, uint32_t E, hipStream_t s);
int launch_agc_init(AgcState *st, uint32_t C, hipStream_t s);
// out row k = in row (C - k) mod C (CSDR_FLAG_DFT_BACKWARD: the analyzer's transform taken as e^{+j}); in != out
int launch_rows_reversed(const void *in, void *out, uint32_t C, size_t row_bytes, hipStream_t s);
// frame-major tails: freqdem straight from Y[nf][M] into channel-major F, or mixed over channels per frame
int launch_transpose_fm(const float2 *Y, float *F, uint32_t M, uint32_t nf, uint32_t c0, uint32_t C, float ref,
                        const float2 *rp_in, float2 *rp_out, hipStream_t s);
int launch_mix_frames(const float2 *Y, void *out, bool fm, uint32_t M, uint32_t nf, uint32_t c0, uint32_t C, float ref,
                      const float2 *rp_in, float2 *rp_out, hipStream_t s);

// ---- ampmodem DSB peak detector (kernels_am.hip): F[c][t] = 2 (|Z| - q_hat), q_hat a one-pole smoother per channel;
// q_in / q_out must be different arrays (ping-pong)
int launch_am(const float2 *Z, float *F, uint32_t C, uint32_t nf, const float *q_in, float *q_out, float alpha, hipStream_t s);

// ---- multi-stage resampler kernels (kernels_resamp.hip) ----
// y[j] = sum_i h[i] w[base0 + 2 j - i], i <= 4m (half-band decimator over a history-prefixed buffer)
int launch_hb_decim(const float2 *w, const float *h, float2 *y, uint32_t ny, uint32_t base0, uint32_t m, hipStream_t s);
// y[k] = (1-mu) F_b(n) + mu F_{b+1}(n) at t = t_first + k delta (Q32.32 over buffer positions)
int launch_resamp_arb(const float2 *w, const float *pfb, float2 *y, uint32_t ny, uint64_t t_first, uint64_t delta, uint32_t npfb,
                      uint32_t P, hipStream_t s);
// w[0..H) <- w[n..n+H)  (keep the last H samples of a history-prefixed buffer; H <= 1024)
int launch_keep_tail(float2 *w, uint32_t H, uint32_t n, hipStream_t s);

// ---- WBFM audio tail (kernels_wbfm.hip) ----
// one direct-form-II section y = b0 v0 + b1 v1 + b2 v2, v0 = x - a1 v1 - a2 v2; pw[k] = A^(16 * 2^k), A = [[-a1,-a2],[1,0]] row-major
struct BiquadParams { float b0, b1, b2, a1, a2; double pw[8][4]; };
BiquadParams design_butter2_lowpass(float fc);                   // iirFilter 2 fc 0 10 10 (Liquid.chs:636-638)
std::vector<float> design_firdecim_kaiser(uint32_t M, uint32_t m, float As);   // firdecim_rrrf_create_kaiser (Liquid.chs:487)
// rows X[C][nf] -> Y[C][nf] (may alias); per-channel state (v1, v2): st_in != st_out
int launch_biquad(const float *X, float *Y, uint32_t C, uint32_t nf, const BiquadParams &p, const float2 *st_in, float2 *st_out,
                  hipStream_t s);
// rows X[C][nf] (nf % M == 0) -> out[C][nf/M]; per-channel history of h_len-1 samples: hist_in != hist_out
int launch_firdecim(const float *X, float *out, uint32_t C, uint32_t nf, uint32_t M, const float *h, uint32_t h_len,
                    const float *hist_in, float *hist_out, hipStream_t s);

// ---- stereo FM decoder (kernels_fmstereo.hip; design in design.cpp) ----
float fir_group_delay(const std::vector<float> &h, float fc);
struct FmsDesign {
    uint32_t N = 0, d = 0;                          // taps of every FIR (round(q / 1350)); wire delay round(groupdelay(pilot FIR, 100 / q))
    std::vector<float> h_pilot, h_audio;            // kaiser(N, 800 / q, 60, 0), kaiser(N, 15000 / q, 60, 0)
    float scale_pilot = 0.f, scale_audio = 0.f;     // 2 fc of each
    uint32_t d_nco = 0;                             // constrain(19000 2 pi / q): the mixers' and the PLL's start step
    float alpha = 0.f, beta = 0.f;                  // PLL gains: 9 / q and sqrtf of it
    BiquadParams bq;                                // iirFilter 2 (5000 / q) 0 10 10
    std::vector<float> h_dec;                       // firdecim_rrrf_create_kaiser(decim, 10, 60)
};
FmsDesign design_fmstereo(double quad_rate, uint32_t decim);
struct FmsBufs {
    const float *hp, *ha, *hdec;                    // taps (device)
    float *xh[2];                                   // [C][Hx] input history (Hx = N - 1 + d), ping-pong
    float *ub[2];                                   // [C][ustride] u with N - 1 history samples in front, ping-pong
    float2 *p;                                      // [C][max_n] pilot branch
    float *lpr, *lr;                                // [C][max_n] L+R; [2C][max_n] L / R planes
    uint2 *pll;                                     // [C] (theta, d_theta)
    float2 *bq;                                     // [2C] de-emphasis state (v1, v2)
    float *dh[2];                                   // [2C][h_dec - 1] decimator history, ping-pong
};
struct FmsLaunch {
    uint32_t C, n, N, d, M, h_dec_len, ustride, theta0, d_nco; int cur;
    float scale_pilot, scale_audio, alpha, beta;
    float b0, b1, b2, a1, a2;
};
// mpx [C][n] -> out [C][2 (n / M)] (L, R interleaved); the kernels' hipEvents bracket when ev != nullptr (6 events)
int launch_fmstereo(const float *mpx, float *out, const FmsBufs &b, const FmsLaunch &l, hipStream_t s, hipEvent_t *ev);
size_t fms_front_lds(uint32_t N, uint32_t d);

// ---- symbol synchroniser (kernels_symsync.hip; design in design.cpp) ----
constexpr uint32_t SYMSYNC_MAX_SUB = 64;             // h_sub_len = 2 k m: the taps of one sub-filter
constexpr uint32_t SYMSYNC_MAX_PFB = 256;            // npfb
constexpr uint32_t SYMSYNC_MAX_BANK = 4096;          // h_sub_len npfb: both banks and the windows stay below 64 KiB of LDS
struct SymsyncState {                                // one stream, kept in HBM between calls
    float tau, bf, rate, del, q_hat, v0, v1;         // v0, v1: the loop filter's direct form II state (v[0], v[1])
    int32_t b;                                       // filterbank index
    uint32_t decim, fault;                           // decim_counter; sticky fault mark
};
struct SymsyncDesign {
    uint32_t k = 0, m = 0, M = 0, k_out = 0, H_len = 0, L = 0;   // L = h_sub_len = H_len / M = 2 k m
    std::vector<float> H, dH;                        // the prototype (f32) and its scaled derivative, H_len each
    std::vector<float> mf, dmf;                      // the banks, tap-major [L][M]: mf[j M + p] = H[p + (L - 1 - j) M]
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, a1 = 0.f, a2 = 0.f, rate_adj = 0.f;   // set_lf_bw, divided by A[0]
    SymsyncState init{};
};
SymsyncDesign design_symsync_kaiser(uint32_t k, uint32_t m, float beta, uint32_t M, float lf_bw, uint32_t k_out);
// symsync_create(k, M, H, H_len) behind the prototype: from d.H (H_len taps) the derivative d.dH and both banks
void symsync_set_prototype(SymsyncDesign &d);
struct SymsyncLaunch {
    uint32_t C, n, cap, L, M, k_out;
    float kf, b0, b1, b2, a1, a2, rate_adj;
};
// x [C][n] -> y [C][cap] (row stride cap), ny [C]; hist [C][L - 1] and st [C] in place; *fault_any = 1 when a stream is faulted
int launch_symsync(const float *x, float *y, uint32_t *ny, const float *mf, const float *dmf, float *hist, SymsyncState *st,
                   uint32_t *fault_any, const SymsyncLaunch &l, hipStream_t s);

// ---- complex symbol synchroniser (kernels_symsyncc.hip; root-Nyquist designs in design.cpp) ----
constexpr uint32_t RNYQUIST_MAX_LEN = 2 * 64 * 8 * 256 + 1;          // taps of a csdr_firdes_rnyquist prototype
// liquid_firdes_prototype(CSDR_FIRFILT_ARKAISER | CSDR_FIRFILT_RRC, k, m, beta, dt): 2 k m + 1 taps, f64, rounded once; empty
// when the ARKAISER bandwidth factor rho_hat falls outside (0, 1)
std::vector<float> design_rnyquist(int ftype, uint32_t k, uint32_t m, float beta, float dt);
// dynamic LDS of k_symsyncc in bytes: both banks and 64 complex windows; a handle is accepted up to SYMSYNCC_MAX_LDS
constexpr size_t SYMSYNCC_MAX_LDS = 65536;
size_t symsyncc_lds_bytes(uint32_t L, uint32_t M);
// x [C][n] CF32 -> y [C][cap] CF32 (row stride cap), ny [C]; hist [C][L - 1] CF32 and st [C] in place, as launch_symsync
int launch_symsyncc(const float2 *x, float2 *y, uint32_t *ny, const float *mf, const float *dmf, float2 *hist, SymsyncState *st,
                    uint32_t *fault_any, const SymsyncLaunch &l, hipStream_t s);

// ---- pskTracker: carrier PLL, T/2 equaliser and PSK decisions (kernels_psktrack.hip; shape and contract functions in
// psktrack_common.h) ----
struct PskLaunch {
    uint32_t C, n, bits, sps, phase, L, mode, delay;     // L = eq_len (0: none); delay = eq_delay in symbols
    float mu, agc_bw, alpha, beta;                       // alpha = pll_bw, beta = sqrtf(pll_bw)
};
// x [C][n] CF32, nx [C] or NULL -> y [C][n] CF32, sym [C][n] or NULL, ny [C]; st_in -> st_out: [C][psk_state_words(L)]
int launch_psktrack(const float2 *x, const uint32_t *nx, float2 *y, uint32_t *sym, uint32_t *ny, const uint32_t *st_in,
                    uint32_t *st_out, const PskLaunch &l, hipStream_t s);

// ---- firhilbf: realToComplex / complexToReal (kernels_firhilb.hip; design in design.cpp) ----
constexpr uint32_t FIRHILB_MAX_M = 16;               // filter semi-length m: 2 m quadrature taps, 2 m pairs of history
// firhilbf_create(m, As): the 2 m quadrature-branch taps hq, oldest sample first
std::vector<float> design_firhilb(uint32_t m, float As);
struct FirhilbLaunch {
    uint32_t n, m, vec;                              // n pairs; vec: both buffers 16-byte aligned (set by the launcher)
    float hq[2 * FIRHILB_MAX_M];
};
// x [2 n] -> y [2 n] floats (pairs: x0, x1 -> re, im when decimating; re, im -> y0, y1 when interpolating); hist_in / hist_out
// [4 m]: the windows pair-interleaved (w1[j], w0[j]) before and after the call; x and y must not overlap
int launch_firhilb(bool interp, const float *x, float *y, const float *hist_in, float *hist_out, FirhilbLaunch l, hipStream_t s);

// ---- M-FSK demodulator (kernels_fskdem.hip; design in design.cpp) ----
constexpr uint32_t FSKDEM_MAX_M = 8;                 // bits per symbol: 2^m tones (this library's limit, not liquid's)
constexpr uint32_t FSKDEM_MAX_K = 2048;              // samples per symbol (liquid's limit)
struct FskdemDesign {
    uint32_t m = 0, k = 0, M = 0, K = 0;             // M = 2^m tones; K: the transform size, k <= K <= max(16, 4 k)
    std::vector<uint32_t> map;                       // demod_map: the bin of tone i, M entries below K
    std::vector<float> W;                            // e^{-2 pi i t / K}, t < K, interleaved (re, im)
    bool repeated = false;                           // two tones share a bin (liquid warns and goes on)
};
FskdemDesign design_fskdem(uint32_t m, uint32_t k, float bandwidth);
struct FskdemLaunch { uint32_t C, n, k, K, M; };
// x [C][n] CF32 -> sym [C][n / k] uint32 and, when energy != nullptr, energy [C][n / k][M] F32; the n mod k samples at the end
// of every row are not read.  W [K] and map [M] are the design's arrays on the device
int launch_fskdem(const float2 *x, uint32_t *sym, float *energy, const float2 *W, const uint32_t *map, const FskdemLaunch &l,
                  hipStream_t s);

// ---- FIR filter (kernels_firfilt.hip; design in design.cpp) ----
constexpr uint32_t FIRFILT_MAX_LEN = 2048;           // taps (this library's limit): tile + halo stay below 64 KiB of LDS
// liquid_firdes_kaiser(n, fc, As, 0): f64, rounded once, window argument 2 t / (n - 1) (the form KAT1 pins); n >= 2
std::vector<float> design_firfilt_kaiser(uint32_t n, float fc, float As);
struct FirfiltLaunch { uint32_t C, n, L; float scale; };
// x [C][n] -> y [C][n] of F32 or (cplx) CF32, y[t] = scale sum_i h[i] x[t - i]; h [L] on the device; hist_in / hist_out
// [C][L - 1]: the samples in front of the call and behind it (different arrays); x and y must not overlap
int launch_firfilt(bool cplx, const void *x, void *y, const float *h, const void *hist_in, void *hist_out, const FirfiltLaunch &l,
                   hipStream_t s);

// ---- order-n IIR filter as a cascade of second-order sections (kernels_iirsos.hip; design in design.cpp) ----
constexpr uint32_t IIRSOS_MAX_SEC = 8, IIRSOS_MAX_ORDER = 2 * IIRSOS_MAX_SEC;
// Butterworth low-pass of order n (1 .. 16) at fc in (0, 0.5) by the bilinear transform with pre-warping: S = ceil(n / 2) sections
// b[3 S], a[3 S] with a0 = 1, one per conjugate pole pair (highest Q first), for odd n a first-order section last; every section
// has unit DC gain.  f64, rounded once
void design_butter_lowpass_sos(uint32_t n, float fc, float *b, float *a);
// one section as the kernel reads it: y = b0 x + k1 v1 + k2 v2 on the state before the sample (k1 = b1 - b0 a1, k2 = b2 - b0 a2,
// from the f32 coefficients in f64, rounded once), pw[k] = A^(16 * 2^k), A = [[-a1, -a2], [1, 0]] row-major
struct IirSosSection { float b0, k1, k2, a1, a2, pad[3]; double pw[8][4]; };
IirSosSection make_iirsos_section(const float *b, float a1, float a2);      // b[3] and a1, a2 already divided by a0
// rows x [C][n] -> y [C][n] of F32 or (cplx) CF32, the same array or disjoint ones; sec [S] and state [C][S] (float2 (v1, v2), for
// cplx float4 (v1.re, v1.im, v2.re, v2.im)) on the device; the state is read and rewritten in place
int launch_iirsos(bool cplx, const void *x, void *y, uint32_t C, uint32_t n, uint32_t S, const IirSosSection *sec, void *state,
                  hipStream_t s);

// ---- GMSK demodulator (kernels_gmskdem.hip; designs in design.cpp) ----
constexpr uint32_t GMSK_MIN_K = 2, GMSK_MAX_K = 64, GMSK_MAX_M = 8;      // this library's limits: L = 2 k m + 1 <= 1025
inline bool gmsk_args_ok(uint32_t k, uint32_t m, float bt)
{
    return k >= GMSK_MIN_K && k <= GMSK_MAX_K && m >= 1 && m <= GMSK_MAX_M && bt >= 0.2f && bt <= 1.0f;
}
// the Gaussian-filtered rectangular frequency pulse, L = 2 k m + 1 taps that sum to one; f64, rounded once
std::vector<float> design_gmsktx(uint32_t k, uint32_t m, float bt);
// this library's receive filter: the r of least sum r^2 whose cascade with the pulse is 1 at the centre and 0 at the 2 m other
// symbol instants of its span; f64, made symmetric, rounded once
std::vector<float> design_gmskrx(uint32_t k, uint32_t m, float bt);
struct GmskdemLaunch { uint32_t C, n, k, m, L, kinv; };                  // n a multiple of k; kinv = 2^32 / k + 1
// x [C][n] CF32 -> sym [C][n / k] uint32 and, when soft != nullptr, soft [C][n / k] F32; h [L] on the device; hist_in / hist_out
// [C][L]: the samples in front of the call and behind it (different arrays)
int launch_gmskdem(const float2 *x, uint32_t *sym, float *soft, const float *h, const float2 *hist_in, float2 *hist_out,
                   const GmskdemLaunch &l, hipStream_t s);

// ---- 2x-oversampled channelizer (kernels_pfb2.hip; launch shape in pfb2_shape.h; design in design.cpp) ----
// Kaiser prototype of firpfbch2_crcf_create_kaiser(ANALYZER, M, m, As) as recalled (unpinned): 2 M m + 1 taps of cutoff fc
// (0: the analyzer's rule, 1 / M), f64, scaled to sum M, rounded once; returns all 2 M m + 1, of which the bank uses the first 2 M m
std::vector<float> design_pfb2_taps(uint32_t M, uint32_t m, float As, float fc);
std::vector<float2> pfb2_twiddles(uint32_t M);                           // e^{+2 pi j k / M}, k < M / 4: f64, rounded once
struct Pfb2Launch { uint32_t frames, par0, tiles, tiles_per_run; };
// x [frames M / 2] CF32 -> y [M][frames] CF32; h [2 m M] and tw [M / 4] on the device; hist_in / hist_out [2 m M - M / 2]: the samples
// in front of the call and behind it (different arrays); parity: frames since the start of the stream, mod 2; x and y must not overlap
int launch_pfb2(const float2 *x, float2 *y, const float *h, const float2 *tw, const float2 *hist_in, float2 *hist_out, uint32_t M,
                uint32_t m, uint32_t frames, uint32_t parity, uint32_t cus, hipStream_t s);

// ---- the synthesizer of the 2x-oversampled bank (kernels_pfb2s.hip; launch shape in pfb2_shape.h) ----
// The prototype is design_pfb2_taps with the synthesizer's cutoff, 0.5 / M; the twiddles are pfb2_twiddles
struct Pfb2sLaunch { uint32_t frames, par0, seen, tiles, tiles_per_run; };
// y [M][frames] CF32 -> x [frames M / 2] CF32; g [2 m M] and tw [M / 4] on the device; hist_in / hist_out [M][4 m - 1]: the input frames
// in front of the call and behind it (different arrays), of which the last `seen` belong to the stream; parity: frames since the
// start of the stream, mod 2; x and y must not overlap
int launch_pfb2s(const float2 *y, float2 *x, const float *g, const float2 *tw, const float2 *hist_in, float2 *hist_out, uint32_t M,
                 uint32_t m, uint32_t frames, uint32_t parity, uint32_t seen, uint32_t cus, hipStream_t s);

// ---- rowResampler: the arbitrary-rate resampler on nchan rows (kernels_rowresamp.hip; launch shape in rowresamp_shape.h) ----
// "csdr rowresamp v1": delta = llround(2^32 / rate), P = 2 m D taps per phase, fc = 0 meaning min(0.515 min(r, 1), 0.49), the bank
// [257][P] = f32(2 fc g[b + 256 j]) of g = firdes_kaiser(256 P + 1, fc / 256, as)
struct RowResampDesign { uint64_t delta = 0; uint32_t P = 0; float fc = 0.f; std::vector<float> bank; };
bool rowresamp_design_args_ok(double rate, uint32_t m, float as_db, float fc);
RowResampDesign design_rowresamp(double rate, uint32_t m, float as_db, float fc);
struct RowResampLaunch { uint64_t delta, T; uint32_t m, n, n_out, tiles, items, items_per_run; };
// x [nchan][n] -> y [nchan][n_out], CF32 (cplx) or F32, n_out = rrs_count(T, delta, n); bank_t: the bank as [P][RRS_BANK_STRIDE], phase b in column rrs_bank_col(b), on the device;
// hist_in / hist_out [nchan][P - 1]: the samples in front of the call and behind it (different arrays); x and y must not overlap
int launch_rowresamp(const void *x, void *y, const float *bank_t, const void *hist_in, void *hist_out, uint64_t delta, uint32_t m,
                     bool cplx, uint32_t nchan, uint32_t n, uint32_t n_out, uint64_t T, uint32_t cus, hipStream_t s);

// ---- time-parallel exact AGC [+ freqdem] tail (kernels_agc_tail.hip) ----
// The state of one tail (a member of AgcTail, chain_tails.h); which kernel a call takes, with which segments and grids: agc_tail_shape.h
struct AgcTailPlan {
    // calls of up to max_nf frames on C rows; the tables come out of mem; cus: compute units of the handle's device.  Reads CSDR_AGC_L,
    // _L_TM, _W, _WGS, _TM and CSDR_CUS
    int init(DeviceBuffers &mem, uint32_t C, uint32_t max_nf, uint32_t cus);
    void reset() { fresh = true; seen = 0; }       // the AGC state was re-initialised: the next call pilots
    int stats(unsigned *checked, unsigned *redone) const;
    bool tm_supported(uint32_t nf) const { return agc_tail_tm_supported(knobs, C, nf); }
    // Z[C][nf] -> out[C][nf] (CF32, or F32 when fm); st (and rp_in -> rp_out when fm) carry the per-channel state
    // tm: Z is a TILE-MAJOR plane -- sample (c, t) at ((t >> 4) C + c) 16 + (t & 15), agc_tail_tm_guard(C) readable elements in front of
    // Z and behind the plane -- which the fused run kernels write for calls tm_supported() accepts (k_agc_spec_tm)
    int run(const float2 *Z, void *out, bool fm, uint32_t nf, AgcState *st, const AgcParams &prm, float fm_ref, const float2 *rp_in,
            float2 *rp_out, hipStream_t s, bool tm);
    uint32_t tm_calls = 0;           // calls that took k_agc_spec_tm since init
private:
    uint32_t C = 0;
    AgcTailKnobs knobs;
    AgcTailSizes sizes{};
    void *d_start = nullptr, *d_end = nullptr, *d_ckpt = nullptr;    // AgcSeg records (kernels_agc_tail.hip): [C][max_seg] x 2, [ckpt_cap]
    AgcState *d_st_tmp = nullptr;    // [C] settled state of the pilot (first call of a stream)
    unsigned *d_stats = nullptr;
    bool fresh = true;               // the AGC state is still inside its create-time transient: the next call runs the pilot
    uint32_t pilot_n = 4096;
    uint64_t seen = 0;               // samples per channel since init / reset
};

// ---- hipEvent bracket around the dominant kernel (CSDR_FLAG_TIME_KERNELS) ----
struct KernelTimer {
    std::vector<hipEvent_t> ev;          // pairs
    size_t used = 0;
    double acc_ms = 0.0; uint32_t launches = 0;
    bool enabled = false;
    // region mode (CSDR_FLAG_TIME_REGION): ONE event in front of the first timed launch and one behind the last, recorded when the
    // total is read; total / launches = the launch cadence of back-to-back calls (kernel + the gap to the next one).  A pair of
    // events around every launch costs the stream 10-20 us per launch on this runtime, which the per-launch mode pays and reports.
    bool region = false, open = false;
    hipEvent_t r0 = nullptr, r1 = nullptr; hipStream_t last = nullptr; uint32_t pending = 0;
    int begin(hipStream_t s) {
        if (!enabled) return 0;
        if (region) {
            if (!open) {
                if (!r0) { CSDR_HIP(hipEventCreate(&r0)); CSDR_HIP(hipEventCreate(&r1)); }
                CSDR_HIP(hipEventRecord(r0, s));
                open = true; pending = 0;
            }
            return 0;
        }
        if (used + 2 > ev.size()) {
            if (ev.size() >= 4096) { int r = drain(); if (r) return r; }
            else for (int i = 0; i < 2; i++) { hipEvent_t e; CSDR_HIP(hipEventCreate(&e)); ev.push_back(e); }
        }
        CSDR_HIP(hipEventRecord(ev[used], s));
        return 0;
    }
    int end(hipStream_t s) {
        if (!enabled) return 0;
        if (region) { last = s; pending++; return 0; }
        CSDR_HIP(hipEventRecord(ev[used + 1], s));
        used += 2;
        return 0;
    }
    int drain() {
        if (region) {
            if (open && pending) {
                CSDR_HIP(hipEventRecord(r1, last));
                CSDR_HIP(hipEventSynchronize(r1));
                float ms = 0.f;
                CSDR_HIP(hipEventElapsedTime(&ms, r0, r1));
                acc_ms += ms; launches += pending;
            }
            open = false; pending = 0;
            return 0;
        }
        for (size_t i = 0; i + 1 < used; i += 2) {
            CSDR_HIP(hipEventSynchronize(ev[i + 1]));
            float ms = 0.f;
            CSDR_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            acc_ms += ms; launches++;
        }
        used = 0;
        return 0;
    }
    void destroy() { for (auto e : ev) (void)hipEventDestroy(e); ev.clear(); used = 0; if (r0) { (void)hipEventDestroy(r0); (void)hipEventDestroy(r1); r0 = r1 = nullptr; } open = false; }
};

}  // namespace csdr

/*
 * csdr.h -- C ABI of the MI355X-native DSP chain that replaces the liquid-dsp
 * FFI calls behind ComposableSDR's Pipe blocks.
 *
 * Every block of the reference is
 *     Pipe { _start :: IO r, _process :: r -> Array a -> IO (Array b), _done :: r -> IO () }
 * (/root/reference/src/ComposableSDR/Types.hs:51-55) whose three fields wrap a
 * liquid-dsp  *_create / *_execute_block / *_destroy  triple.  Each object
 * below exports the same triple at the same (chunk) granularity:
 *     int csdr_X_create (..., csdr_X **out);      <- _start
 *     int csdr_X_process(csdr_X *, in, n, out);   <- _process (one whole chunk)
 *     int csdr_X_destroy(csdr_X *);               <- _done
 * Conventions:
 *   - return 0 on success, <0 on error (so the Haskell side can reuse
 *     Common.hs:32-33 `try`); never exit(); csdr_last_error() gives the text.
 *     liquid-dsp 1.3.2 aborts the process on a bad configuration instead.
 *   - in/out buffers are caller-owned and only touched during the call; CF32 is
 *     interleaved little-endian float32 (re, im) = Types.hs:82-88.
 *   - handles are opaque, single-threaded, independent of each other; all
 *     stream state (DC-blocker v1, NCO phase, filterbank windows, per-channel
 *     AGC / freqdem state) lives in the handle, so results do not depend on how
 *     the stream is chunked.
 *   - *_process takes host pointers and blocks; *_process_device takes device
 *     pointers (HBM-resident data) and enqueues on a hipStream_t without
 *     synchronising.
 * All compute runs in hand-written HIP kernels for gfx950.  There is no CPU
 * fallback: with no usable GPU every create returns CSDR_ERR_NODEV.
 */
#ifndef CSDR_H
#define CSDR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libcsdr_hip.so is built with -fvisibility=hidden: the declarations between this push and the
 * pop at the end of the file are the library's whole dynamic symbol table (what a Haskell
 * `foreign import ccall` can bind); the C++ internals behind them are not exported. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define CSDR_OK            0
#define CSDR_ERR_INVALID  (-1)  /* bad argument / configuration                         */
#define CSDR_ERR_HIP      (-2)  /* HIP runtime error (text in csdr_last_error)          */
#define CSDR_ERR_NODEV    (-3)  /* no gfx950 device visible                              */
#define CSDR_ERR_SIZE     (-4)  /* chunk length not a multiple of the channel count, or
                                   larger than the handle was created for                */
#define CSDR_ERR_NOMEM    (-5)
#define CSDR_ERR_BUSY     (-6)  /* csdr_chain_submit: CSDR_CHAIN_INFLIGHT chunks already pending */

#define CSDR_DEMOD_NONE 0u      /* DeNo: per-channel CF32 out (SoapySDR.hs:236-243)      */
#define CSDR_DEMOD_FM   1u      /* DeNBFM kf: freqdem, F32 out (SoapySDR.hs:244-251)     */
#define CSDR_DEMOD_WBFM 3u      /* DeWBFM decim: firDecimator decim . iirDeemph . fmDemodulator 0.6,
                                   F32 out, n_in/channels/decim samples per channel
                                   (SoapySDR.hs:252-259, Liquid.chs:653-656)              */
#define CSDR_DEMOD_AM   2u      /* DeAM: ampmodem DSB peak detector, F32 out
                                   (SoapySDR.hs:265-272, Liquid.chs:439-469)              */

/* cfg.flags */
#define CSDR_FLAG_TIME_KERNELS 1u   /* bracket the dominant kernel with hipEvents         */
#define CSDR_FLAG_FORCE_GENERIC 2u  /* use the any-M multi-kernel path even where a fused
                                       kernel exists (for A/B tests)                      */
#define CSDR_FLAG_QUIET 4u          /* do not print the configuration at create           */
#define CSDR_FLAG_AGC_SEQUENTIAL 8u /* run the per-channel AGC as one lane per channel instead of
                                       the time-parallel verified tail; both give bit-identical
                                       output (for A/B tests)                                */
#define CSDR_FLAG_NO_MIX_IDENTITY 16u /* DeNo --mix over all channels of the any-M route: sum_k Y[k] = M * X[0] (the sum of all
                                        * DFT bins of a frame is M times its first input), so the product path computes the
                                        * DC blocker on the whole stream and the FIR of polyphase branch 0 only.  Set this flag
                                        * to run the full bank + DFT + channel sum instead (same result to f32 rounding).      */

#define CSDR_FLAG_TIME_REGION 32u   /* time the dominant kernel over a REGION instead of per launch: one hipEvent in front of the
                                     * first timed launch after the last csdr_chain_kernel_time() and one behind the last, recorded
                                     * when the total is read.  total / launches is then the launch cadence of back-to-back calls
                                     * (kernel + the gap to the next launch); it includes whatever else the call puts on the stream
                                     * between two timed launches, so it is a per-kernel figure only for one-kernel steps.  Per-launch
                                     * event pairs (CSDR_FLAG_TIME_KERNELS alone) cost the stream 10-20 us per launch.           */

#define CSDR_FLAG_TAIL_ONLY 64u     /* the handle is the per-channel TAIL of the chain alone: `automaticGainControl` (with the mute
                                     * rule) [-> `fmDemodulator kf`] [-> `mix`] on `channels` independent rows (Trans.hs:124-129 `mux`,
                                     * SoapySDR.hs:249).  process(): in = a channel-major CF32 plane [channels][nf] (n_in = channels *
                                     * nf samples: what a DeNo chain writes), out = [channels][nf] CF32 / F32 ([nf] with mix).  For the
                                     * hybrid multi-GPU partition: DC blocker, pre-mix, FIR and DFT run time-sharded, one
                                     * all-to-all turns time stripes into channel shards, every rank runs this tail on its channels for
                                     * the whole time span.  Needs agc_threshold_db != 0; dc_block, chan_*, pfb_* are ignored.         */

#define CSDR_FLAG_DFT_BACKWARD 128u /* The direction of firpfbch_crcf_analyzer_execute's transform (Liquid.chs:843) is recalled, not pinned by
                                     * anything in the reference (hard part 1): the library computes the FORWARD DFT
                                     * out[k] = sum_j X[j] e^{-j 2 pi jk/M}.  With this flag the handle delivers the other possible
                                     * convention, out[k] = sum_j X[j] e^{+j 2 pi jk/M} = forward bin (M - k) mod M: output row k (file
                                     * _ch<k+1>) is the forward chain's row (M - k) mod M, every per-channel tail (AGC, demod) unchanged
                                     * on its row.  One extra pass over the OUTPUT (a row permutation behind the fused kernels); whole-band
                                     * handles only (channel shards: CSDR_ERR_INVALID); with mix the sum over all channels is the same set
                                     * of terms, so only the fold order differs (no-op).  Should a diff against a real liquid-dsp 1.3.2
                                     * show the backward convention, this flag becomes the default and nothing else changes.        */

const char *csdr_last_error(void);
int  csdr_device_count(void);
/* library / build identification: "csdr-hip gfx950 <version>" */
const char *csdr_version(void);

/* ------------------------------------------------------------------------ *
 * dcBlocker  (Liquid.chs:575-589)
 *   replaces iirfilt_crcf_create_dc_blocker / _execute_block / _destroy
 *   (imports at Liquid.chs:550-567).  y = DC-blocked x, same length.
 * ------------------------------------------------------------------------ */
typedef struct csdr_dcblock csdr_dcblock;
int csdr_dcblock_create(float alpha, uint32_t max_samples, csdr_dcblock **out);
int csdr_dcblock_process(csdr_dcblock *h, const float *x_cf32, uint32_t n, float *y_cf32);
int csdr_dcblock_process_device(csdr_dcblock *h, const void *d_x, uint32_t n, void *d_y, void *stream);
int csdr_dcblock_destroy(csdr_dcblock *h);

/* ------------------------------------------------------------------------ *
 * mixDown / mixUp  (Liquid.chs:782-809)
 *   replaces nco_crcf_create(LIQUID_VCO) + set_frequency + mix_block_down/up
 *   + destroy (imports at Liquid.chs:746-780).  freq in rad/sample.
 * ------------------------------------------------------------------------ */
typedef struct csdr_nco csdr_nco;
int csdr_nco_create(float freq, uint32_t max_samples, csdr_nco **out);
int csdr_nco_mix_down(csdr_nco *h, const float *x_cf32, uint32_t n, float *y_cf32);
int csdr_nco_mix_up(csdr_nco *h, const float *x_cf32, uint32_t n, float *y_cf32);
int csdr_nco_get_words(const csdr_nco *h, uint32_t *theta, uint32_t *d_theta);
int csdr_nco_destroy(csdr_nco *h);

/* ------------------------------------------------------------------------ *
 * automaticGainControl tres  (Liquid.chs:693-728), `nchan` independent
 * instances as created by mux / distribute_ (Trans.hs:106-129).
 *   replaces agc_crcf_create + set_bandwidth 0.1 + set_signal_level 1e-3 +
 *   squelch_enable + squelch_set_threshold tres + squelch_set_timeout 1000,
 *   and per sample execute_block(n=1) + squelch_get_status + get_rssi with the
 *   reference's mute rule "status /= SIGNALHI => 0" (imports :660-691).
 *   x, y are channel-major [nchan][n] CF32.
 * ------------------------------------------------------------------------ */
typedef struct csdr_agc csdr_agc;
int csdr_agc_create(float threshold_db, uint32_t nchan, uint32_t max_samples, csdr_agc **out);
int csdr_agc_process(csdr_agc *h, const float *x_cf32, uint32_t n, float *y_cf32);
int csdr_agc_destroy(csdr_agc *h);

/* ------------------------------------------------------------------------ *
 * fmDemodulator kf  (Liquid.chs:303-334), `nchan` independent instances.
 *   replaces freqdem_create / freqdem_demodulate_block / freqdem_destroy
 *   (imports :305-315).  x is [nchan][n] CF32, m is [nchan][n] F32.
 * ------------------------------------------------------------------------ */
typedef struct csdr_freqdem csdr_freqdem;
int csdr_freqdem_create(float kf, uint32_t nchan, uint32_t max_samples, csdr_freqdem **out);
int csdr_freqdem_process(csdr_freqdem *h, const float *x_cf32, uint32_t n, float *m_f32);
int csdr_freqdem_destroy(csdr_freqdem *h);

/* ------------------------------------------------------------------------ *
 * iirFilter n fc f0 ap as  (Liquid.chs:629-638) = iirfilt_rrrf_create_prototype(BUTTER, LOWPASS,
 * SOS, n, fc, f0, ap, as) (imports :593-611), `nchan` independent real-valued instances.
 * Only what the reference instantiates is built: order 2 (the WBFM de-emphasis,
 * Liquid.chs:655); other orders return CSDR_ERR_INVALID.  f0 / ap / as do not enter a
 * Butterworth low-pass and are ignored, as in liquid.  x, y are [nchan][n] F32.
 * firDecimator m  (Liquid.chs:485-501) = firdecim_rrrf_create_kaiser(m, 10, 60) (imports
 * :473-483): x is [nchan][n] F32 with n % m == 0 (the reference's `div`), y is [nchan][n/m].
 * Arithmetic recalled from liquid-dsp 1.3.2 (unpinned).
 * ------------------------------------------------------------------------ */
typedef struct csdr_iirfilt csdr_iirfilt;
int csdr_iirfilt_create(uint32_t order, float fc, float f0, float ap, float as_db, uint32_t nchan, uint32_t max_samples,
                        csdr_iirfilt **out);
int csdr_iirfilt_process(csdr_iirfilt *h, const float *x_f32, uint32_t n, float *y_f32);
int csdr_iirfilt_destroy(csdr_iirfilt *h);
typedef struct csdr_firdecim csdr_firdecim;
int csdr_firdecim_create(uint32_t decim, uint32_t nchan, uint32_t max_samples, csdr_firdecim **out);
int csdr_firdecim_process(csdr_firdecim *h, const float *x_f32, uint32_t n, float *y_f32);
int csdr_firdecim_destroy(csdr_firdecim *h);

/* ------------------------------------------------------------------------ *
 * resampler r as  (Liquid.chs:56-117): rate r = bandwidth / samplerate, as = 60 dB
 * (SoapySDR.hs:190-194).
 *   replaces msresamp_crcf_create / _print / _get_rate / _execute / _destroy
 *   (imports :58-73).  Variable-length output like msresamp_crcf_execute's
 *   out-count pointer (:79-98): the caller provides csdr_resamp_max_out(h, n_in)
 *   samples of room (= the reference's 2*ceil(r*nx), :81).
 *   Structure = liquid-dsp's msresamp (half-band decimators + one arbitrary-rate
 *   polyphase stage); liquid's internal filter parameters are not recoverable from
 *   the reference, so they are fixed by this library: unpinned.
 *   rate == 0: pass-through (the reference's nullPtr resampler, :100-103);
 *   rate > 2: CSDR_ERR_INVALID.  CSDR_QUIET in the environment silences the print.
 * ------------------------------------------------------------------------ */
typedef struct csdr_resamp csdr_resamp;
int      csdr_resamp_create(float rate, float as_db, uint32_t max_in, csdr_resamp **out);
float    csdr_resamp_get_rate(const csdr_resamp *h);
uint32_t csdr_resamp_max_out(const csdr_resamp *h, uint32_t n_in);
int      csdr_resamp_process(csdr_resamp *h, const float *x_cf32, uint32_t n_in, float *y_cf32, uint32_t *n_out);
int      csdr_resamp_process_device(csdr_resamp *h, const void *d_x, uint32_t n_in, void *d_y, uint32_t *n_out, void *stream);
int      csdr_resamp_destroy(csdr_resamp *h);

/* ------------------------------------------------------------------------ *
 * amDemodulator  (Liquid.chs:439-469), `nchan` independent instances.
 *   replaces ampmodem_create(0.8, LIQUID_AMPMODEM_DSB, 0) / ampmodem_demodulate_block /
 *   ampmodem_destroy (imports :441-450).  x is [nchan][n] CF32, m is [nchan][n] F32.
 *   Arithmetic = liquid-dsp 1.3.2's non-coherent peak detector as recalled (unpinned):
 *   t = |x|, q <- 0.01 t + 0.99 q, m = 2 (t - q); mod_index is accepted and unused, as there.
 * ------------------------------------------------------------------------ */
typedef struct csdr_ampdem csdr_ampdem;
int csdr_ampdem_create(float mod_index, uint32_t nchan, uint32_t max_samples, csdr_ampdem **out);
int csdr_ampdem_process(csdr_ampdem *h, const float *x_cf32, uint32_t n, float *m_f32);
int csdr_ampdem_destroy(csdr_ampdem *h);

/* ------------------------------------------------------------------------ *
 * stereoFMDecoder quadRate decim  (Liquid.chs:959-1078; DeFMS decim fmt, SoapySDR.hs:261-264),
 * `nchan` independent streams.  replaces the reference's pilot-branch NCOs + firfilt_crcf
 * (mixUp ncoF . firPilot . mixDown ncoF), the pilot PLL (two nco_crcf + pll_step / step,
 * Liquid.chs:959-989), the L+R / L-R firfilt_crcf, the L/R matrix, and per channel
 * iirFilter 2 (5000/q) 0 10 10 + firDecimator decim (Liquid.chs:1005-1046).
 *   quad_rate q: the MPX sample rate (the app's outBW); every FIR has round(q/1350) taps;
 *   q in [40e3, 2.7e6].  mpx is [nchan][n] F32 (freqdem output), lr is [nchan][2*floor(n/decim)]
 *   F32 interleaved L, R, L, R ...; *n_out = nchan * 2 * floor(n/decim) elements.
 *   Any n <= max_samples is accepted.  Everything up to the de-emphasis is stream-continuous;
 *   the decimator consumes floor(n/decim)*decim samples per call and drops the rest, as the
 *   reference's firDecim `div` does (Liquid.chs:495-497).
 * DEVIATION: the reference's `delay d` (Trans.hs:86-104) lags the wire by d more
 * samples per chunk and pairs its buffered tail with a zero wire at the end; this object applies
 * the evident intent instead: the wire is x[t - d] (0 before the stream start), every input
 * sample yields one output pair, no end-of-stream flush (the last d wire samples are not emitted).
 * d = round(fir_group_delay(pilot FIR, 100/q)) (csdr_fmstereo_get_delay).  liquid-dsp's Kaiser
 * design, group delay and PLL arithmetic are recalled from 1.3.2: unpinned.
 * ------------------------------------------------------------------------ */
typedef struct csdr_fmstereo csdr_fmstereo;
int csdr_fmstereo_create(float quad_rate, uint32_t decim, uint32_t nchan, uint32_t max_samples, csdr_fmstereo **out);
int csdr_fmstereo_process(csdr_fmstereo *h, const float *mpx, uint32_t n, float *lr, uint32_t *n_out);
int csdr_fmstereo_process_device(csdr_fmstereo *h, const void *d_mpx, uint32_t n, void *d_lr, uint32_t *n_out, void *stream);
int csdr_fmstereo_reset(csdr_fmstereo *h);                       /* back to the state right after create            */
uint32_t csdr_fmstereo_get_delay(const csdr_fmstereo *h);        /* d, the wire delay in samples                    */
uint32_t csdr_fmstereo_get_taps_len(const csdr_fmstereo *h);     /* N, the taps of every FIR                        */
/* the PLL's uint32 words (ncoPE theta, d_theta) of stream `chan` after the last call (synchronises) */
int csdr_fmstereo_get_pll(csdr_fmstereo *h, uint32_t chan, uint32_t *theta, uint32_t *d_theta);
/* with CSDR_DIAG=1 CSDR_FMS_TIME=1 at create: hipEvent times of the last call's five kernels in us
 * (front, pll, back, deemph, decim); synchronises.  CSDR_ERR_INVALID when timing is off. */
int csdr_fmstereo_kernel_times(csdr_fmstereo *h, float *us5);
int csdr_fmstereo_destroy(csdr_fmstereo *h);

/* ------------------------------------------------------------------------ *
 * symSyncR k m beta npfb  (Liquid.chs:244-282; fmDemWithSync k = symSyncR k 4 0 64 . fmDemodulator (0.02 k),
 * Liquid.chs:431-437; DeNBFMSync k, SoapySDR.hs:273-280), `nchan` independent F32 streams.  Replaces
 * symsync_rrrf_create_kaiser(k, m, beta, npfb) + set_lf_bw(lf_bw) + set_output_rate(k_out) + symsync_rrrf_execute
 * through syncSym (Liquid.chs:196-221; the reference passes lf_bw 0.05 and k_out 2).  liquid-dsp 1.3.2 as recalled:
 * unpinned.
 *   design: H_len = 2 npfb k m + 1; H = liquid_firdes_kaiser(H_len, 0.75 / (k npfb), 40, 0) 2 0.75 (f64, rounded once;
 *     beta ignored); dH[i] = H[i+1] - H[i-1] wrapping at both ends, scaled by 0.06 / max |H[i] dH[i]|; two firpfb banks of
 *     npfb sub-filters of h_sub_len = H_len / npfb = 2 k m taps, sub-filter p = H[p + j npfb] reversed (newest sample
 *     meets H[p]).  Loop filter (set_lf_bw bt): B = {0.22 bt, 0, 0}, A = {1 - 0.5 (1 - bt), -0.495 (1 - bt), 0} / A[0]
 *     in direct form II; rate_adjustment 0.5 bt.  Initial rate = del = k / k_out, tau = bf = b = 0, decim_counter 0.
 *   per input sample: push x; while b < npfb { y = MF_b / k; if decim_counter == k_out { decim_counter = 0;
 *     q = clip(MF_b dMF_b, -1, 1); q_hat = iir(q); rate += rate_adjustment q_hat; del = rate + q_hat }
 *     decim_counter++; tau += del; bf = tau npfb; b = roundf(bf) }; then tau -= 1, bf -= npfb, b -= npfb.
 *   Arithmetic: plain f32 without contraction; each dot product summed oldest sample first, starting from the first
 *     product; roundf; a correctly rounded / k.  The output does not depend on the chunking, bit for bit.
 *   Limits (create, else CSDR_ERR_INVALID): k >= k_out >= 1, m >= 1, 2 k m <= 64, npfb in [1, 256], 2 k m npfb <= 4096,
 *     lf_bw in [0, 1].
 *   x is [nchan][n]; y is [nchan][n] (row stride n: the reference's ny = nx buffer), row c holding ny[c] outputs
 *     (about n k_out / k).
 * DEVIATION: a stream that would take del <= 0, index a bank outside [0, npfb) or write more than n
 * outputs in one call (the reference loops for ever or overruns its buffer there) stops producing for the call and is
 * marked faulted; the mark is sticky until reset, a faulted stream yields 0 outputs, and csdr_symsync_process returns
 * CSDR_ERR_SIZE (csdr_symsync_get_state reports it per stream).
 * ------------------------------------------------------------------------ */
typedef struct csdr_symsync csdr_symsync;
int csdr_symsync_create(uint32_t k, uint32_t m, float beta, uint32_t npfb, float lf_bw, uint32_t k_out, uint32_t nchan,
                        uint32_t max_samples, csdr_symsync **out);
int csdr_symsync_process(csdr_symsync *h, const float *x, uint32_t n, float *y, uint32_t *ny);
/* device buffers: d_x [nchan][n] F32, d_y [nchan][n] F32, d_ny [nchan] uint32; enqueued on `stream`, no synchronisation
 * (a fault shows in csdr_symsync_get_state or the next csdr_symsync_process) */
int csdr_symsync_process_device(csdr_symsync *h, const void *d_x, uint32_t n, void *d_y, void *d_ny, void *stream);
int csdr_symsync_reset(csdr_symsync *h);                         /* back to the state right after create            */
/* tau, rate, del, q_hat of stream `chan` after the last call (synchronises); CSDR_ERR_SIZE when the stream is faulted */
int csdr_symsync_get_state(csdr_symsync *h, uint32_t chan, float *tau, float *rate, float *del, float *q_hat);
uint32_t csdr_symsync_get_taps_len(const csdr_symsync *h);       /* h_sub_len = 2 k m                                */
/* both banks as the kernel holds them, tap-major [h_sub_len][npfb]: mf[j npfb + p] = H[p + (h_sub_len - 1 - j) npfb] */
int csdr_symsync_get_taps(const csdr_symsync *h, float *mf, float *dmf);
int csdr_symsync_destroy(csdr_symsync *h);

/* ------------------------------------------------------------------------ *
 * symSyncC m k  (Liquid.chs:177-242), `nchan` independent CF32 streams: liquid's symsync_crcf, which is symsync_rrrf's
 * macro on complex samples with the same real taps and the same loop.  The reference creates it with
 * symsync_crcf_create_rnyquist(LIQUID_FIRFILT_ARKAISER, k, m, 0.5, 32) and leaves lf_bw (0.01) and the output rate (1) at
 * symsync_create's defaults (Liquid.chs:223-232).  There is no new handle: a csdr_symsync handle learns new banks through
 * two setters and complex rows through two process entry points.  liquid-dsp 1.3.2 as recalled: unpinned,
 * except the two prototype designs.
 *   csdr_firdes_rnyquist (no GPU needed): liquid_firdes_prototype(ftype, k, m, beta, dt), n = 2 k m + 1 taps, evaluated in
 *     f64 and rounded once.
 *     CSDR_FIRFILT_RRC: liquid_firdes_rrcos, the closed form (pinned by mathematics).  z = (i + dt) / k - m;
 *       z = 0: 1 - beta + 4 beta / pi;  |z| = 1 / (4 beta) (taken as |1 - 16 beta^2 z^2| < 1e-8):
 *       (beta / sqrt 2) [(1 + 2 / pi) sin(pi / (4 beta)) + (1 - 2 / pi) cos(pi / (4 beta))];  otherwise
 *       [sin(pi z (1 - beta)) + 4 beta z cos(pi z (1 + beta))] / [pi z (1 - 16 beta^2 z^2)].  No further normalisation.
 *     CSDR_FIRFILT_ARKAISER: liquid_firdes_arkaiser as recalled, the r-Kaiser filter with an approximated bandwidth factor:
 *       rho_hat = c0 + c1 ln beta + c2 ln^2 beta, c0 = 0.762886 + 0.067663 ln m, c1 = 0.065515, c2 = ln(1 - 0.088 m^-1.6);
 *       kf = 0.5 (1 + beta (1 - rho_hat)) / k, del = beta rho_hat / k; h = csdr_firdes_kaiser's function (n, kf, As) with t
 *       shifted by dt, scaled to sum h^2 = k.  Pinned by the property it approximates: rho_hat lies within 0.02 of the rho
 *       that minimises the inter-symbol interference of h * h, at no more than 3 times the least rms ISI
 *       (tests/test_rnyquist_cpu.py).  DEVIATION: As = 14.26 del n + 7.95, Kaiser's length formula solved for As, where
 *       liquid bisects an estimate.
 *     CSDR_ERR_INVALID: another ftype, k < 2, m < 1, n > 2 64 8 256 + 1, beta outside (0, 1], dt outside [-1, 1], h NULL,
 *       and an ARKAISER rho_hat outside (0, 1) (liquid switches to a second approximation there, not reproduced).
 *   csdr_symsync_set_taps: liquid's symsync_create(k, npfb, H, H_len) behind create.  H_len must be the handle's
 *     2 npfb k m + 1 (else CSDR_ERR_INVALID; so are NULL and taps that are not finite or all zero).  From H it builds what
 *     create builds from its Kaiser prototype (dH with the wrap-around ends, the 0.06 / max |H dH| scale in f32, the two
 *     reversed tap-major banks), uploads them and puts the handle back to its state right after create (synchronises).
 *     csdr_symsync_get_taps reports the new banks.
 *   csdr_symsync_set_rnyquist: symsync_create_rnyquist(ftype, k, m, beta, npfb) = csdr_firdes_rnyquist(ftype, k npfb, m,
 *     beta, 0, H) + csdr_symsync_set_taps.  F32 and CF32 rows both run on whatever banks the handle holds.
 *   Sample type: the first process call after create, reset, set_taps or set_rnyquist fixes whether the handle takes F32
 *     rows (csdr_symsync_process*) or CF32 rows (csdr_symsync_process_c*); the other kind of call is CSDR_ERR_INVALID and
 *     touches nothing.  The complex windows are allocated by the first complex call.
 *   csdr_symsync_process_c*: x is [nchan][n] interleaved CF32, y is [nchan][n] CF32 (row stride n), row c holding ny[c]
 *     outputs.  Per input sample as csdr_symsync above with MF_b and dMF_b complex: y = (MF.re / k, MF.im / k) and
 *     q = clip(MF.re dMF.re + MF.im dMF.im, -1, 1) = Re(conj(MF) dMF).
 *   Arithmetic: plain f32 without contraction; MF.re and MF.im (and dMF's) are independent sums, oldest sample first,
 *     starting from the first product; q is two rounded products and one add; the rest as for F32 rows.  The output does
 *     not depend on the chunking, on nchan or on host versus device entry, bit for bit.  The fault rule is the F32 rows'.
 *   Limit of the complex calls (CSDR_ERR_INVALID otherwise; F32 rows are not affected): both banks and 64 complex windows
 *     share 64 KiB of LDS, 8 (2 k m) npfb + 512 ((2 k m + 31) | 1) <= 65536 bytes.  Every handle with 2 k m <= 64 and
 *     npfb <= 32 fits, and so does (k, m, npfb) = (4, 4, 64).
 * ------------------------------------------------------------------------ */
#define CSDR_FIRFILT_ARKAISER 7   /* liquid's numbers, as Liquid.chs:225 and :160 pass them */
#define CSDR_FIRFILT_RRC      9
int csdr_firdes_rnyquist(int ftype, uint32_t k, uint32_t m, float beta, float dt, float *h);   /* n = 2 k m + 1 taps */
/* Liquid.chs:177-242: liquid's symsync_crcf_create(k, npfb, H, H_len) on an existing handle */
int csdr_symsync_set_taps(csdr_symsync *h, const float *H, uint32_t H_len);
/* Liquid.chs:177-242: symsync_crcf_create_rnyquist(ftype, k, m, beta, npfb) on an existing handle (:228) */
int csdr_symsync_set_rnyquist(csdr_symsync *h, int ftype, float beta);
/* Liquid.chs:177-242: symsync_crcf_execute (:188-191, :242); x, y interleaved CF32 [nchan][n] */
int csdr_symsync_process_c(csdr_symsync *h, const float *x, uint32_t n, float *y, uint32_t *ny);
/* Liquid.chs:177-242, device buffers: d_x, d_y [nchan][n] CF32, d_ny [nchan] uint32; enqueued on `stream`, no synchronisation */
int csdr_symsync_process_c_device(csdr_symsync *h, const void *d_x, uint32_t n, void *d_y, void *d_ny, void *stream);

/* ------------------------------------------------------------------------ *
 * realToComplex / complexToReal  (Liquid.chs:503-546; the audio-file source mixUp (2 pi 0.5) . realToComplex,
 * Source.chs:273-307).  Replaces firhilbf_create(m, As) (firhilbCreate passes 5, 60.0, Liquid.chs:520-525) with
 * firhilbf_decim_execute_block (Liquid.chs:530-534) and firhilbf_interp_execute_block (Liquid.chs:539-543).
 * liquid-dsp 1.3.2 as recalled: unpinned.
 *   design: h = liquid_firdes_kaiser(4 m + 1, 0.25, As, 0) (f64, rounded once); hc[i] = h[i] e^{j pi (i - 2 m) / 2};
 *     the 2 m quadrature taps hq[j] = Im hc[4 m - i], i = 2 j + 1.
 *   state: two windows w0, w1 of 2 m floats, zero after create / reset; a push appends the newest, index 0 is the oldest.
 *   decimator, per input pair (x0, x1): push x0 to w1, yq = sum_j hq[j] w1[j]; push x1 to w0, yi = w0[m - 1]; out yi + j yq.
 *   interpolator, per input x: push Im x to w0, y[0] = w0[m - 1]; push Re x to w1, y[1] = sum_j hq[j] w1[j].
 *   Arithmetic: plain f32 without contraction, the sum taken j = 0 .. 2 m - 1 starting from the first product.  The output
 *     does not depend on the chunking, bit for bit.  One handle may be driven in both directions; the windows are shared.
 *   Limits (create, else CSDR_ERR_INVALID): m in [2, 16], As > 0, max_samples <= 2^30 (0 means 4096).
 *   n counts complex samples: any n <= max_samples, 0 included.  Input and output buffers must not overlap.
 * ------------------------------------------------------------------------ */
typedef struct csdr_firhilb csdr_firhilb;
int csdr_firhilb_create(uint32_t m, float as_db, uint32_t max_samples, csdr_firhilb **out);
/* firhilbf_decim_execute_block (Liquid.chs:530-534): 2 n reals in, n complex out */
int csdr_firhilb_decim(csdr_firhilb *h, const float *x_f32, uint32_t n, float *y_cf32);
/* firhilbf_interp_execute_block (Liquid.chs:539-543): n complex in, 2 n reals out */
int csdr_firhilb_interp(csdr_firhilb *h, const float *x_cf32, uint32_t n, float *y_f32);
/* device buffers of 2 n floats each; enqueued on `stream`, no synchronisation */
int csdr_firhilb_decim_device(csdr_firhilb *h, const void *d_x, uint32_t n, void *d_y, void *stream);
int csdr_firhilb_interp_device(csdr_firhilb *h, const void *d_x, uint32_t n, void *d_y, void *stream);
int csdr_firhilb_reset(csdr_firhilb *h);                         /* back to the state right after create            */
uint32_t csdr_firhilb_get_taps_len(const csdr_firhilb *h);       /* 2 m                                              */
int csdr_firhilb_get_taps(const csdr_firhilb *h, float *hq);     /* the quadrature taps, oldest sample first         */
int csdr_firhilb_destroy(csdr_firhilb *h);

/* ------------------------------------------------------------------------ *
 * fskDemodulator m k bw  (Liquid.chs:336-382), `nchan` independent CF32 streams: non-coherent M-FSK, M = 2^m tones,
 * k samples per symbol, tones spread over +- bw.  Replaces fskdem_create(m, k, bw) / fskdem_demodulate per symbol /
 * fskdem_destroy (imports :338-348) and the energies of fskdem_get_symbol_energy.  liquid-dsp 1.3.2 as recalled:
 * unpinned.
 *   design (all f32): M2 = 0.5 (M - 1), df = bw / M2; K = the K_hat in [k, max(16, 4 k)] with the smallest
 *     |roundf(v) - v|, v = 0.5 df K_hat (the first of equals; the search stops at the first error below 1e-6);
 *     demod_map[i] = roundf(idx < 0 ? idx + K : idx) mod K, idx = ((i - M2) bw / M2) K.  Two tones may share a bin: as in
 *     liquid that is a warning on stderr (silenced by CSDR_QUIET in the environment), not an error.
 *   per symbol of k samples: X[b] = sum_{j < k} x[j] e^{-2 pi i b j / K} (the K-point forward DFT of the zero-padded
 *     symbol) at the M mapped bins; E[s] = |X[demod_map[s]]|; the symbol is the first s with the largest E
 *     (s == 0 || E[s] > max so far), so an all-zero symbol gives 0.
 *   Arithmetic: plain f32 without contraction.  The phasors come from a table W[t] = e^{-2 pi i t / K}, t < K, evaluated
 *     in f64 and rounded once, indexed by (b j) mod K; a product is four multiplies, one subtraction and one addition;
 *     each sum starts at +0 and takes j = 0 .. k - 1 in that order; E = sqrtf(re re + im im), correctly rounded.
 *   Chunk rule (Liquid.chs:367-376: `n div k` symbols, the throw commented out): a call of n samples per row yields
 *     n / k symbols per row and drops the last n mod k samples of every row.  The handle carries nothing from call to
 *     call, so a stream cut at symbol boundaries gives the same bits as one call, and any other cut loses the tails.
 *   Limits (create, else CSDR_ERR_INVALID): m >= 1, k in [2, 2048], 0 < bw < 0.5 (where liquid exits) and m <= 8 (this
 *     library's).  n > max_samples: CSDR_ERR_SIZE (max_samples 0 means 4096).
 *   x is [nchan][n] CF32 (what a DeNo chain writes); sym is [nchan][n / k] uint32; energy, when not NULL, is
 *     [nchan][n / k][M] F32; *n_out = nchan * (n / k).
 * ------------------------------------------------------------------------ */
typedef struct csdr_fskdem csdr_fskdem;
int csdr_fskdem_create(uint32_t m, uint32_t k, float bandwidth, uint32_t nchan, uint32_t max_samples, csdr_fskdem **out);
int csdr_fskdem_process(csdr_fskdem *h, const float *x_cf32, uint32_t n, uint32_t *sym, float *energy, uint32_t *n_out);
/* device buffers as above; d_energy may be NULL; enqueued on `stream`, no synchronisation */
int csdr_fskdem_process_device(csdr_fskdem *h, const void *d_x, uint32_t n, void *d_sym, void *d_energy, void *stream);
/* K and the M entries of demod_map (either pointer may be NULL) */
int csdr_fskdem_get_design(const csdr_fskdem *h, uint32_t *K, uint32_t *demod_map);
int csdr_fskdem_destroy(csdr_fskdem *h);

/* ------------------------------------------------------------------------ *
 * firFilterCKaiser n fc as mu / firFilterC f / firFilterR f  (Liquid.chs:868-916, 955-957), `nchan` independent rows of
 * F32 (firfilt_rrrf) or CF32 (firfilt_crcf) samples, real taps.  Replaces firfilt_crcf_create_kaiser + set_scale (2 fc)
 * (firfiltCreateCKaiser, :889-895), firfilt_*_execute_block, firfilt_crcf_groupdelay (:879) and liquid_firdes_kaiser.
 *   filter: L taps h[0 .. L-1], a scale s: y[t] = s * sum_{i < L} h[i] x[t - i].  x[t < 0] is the row's history: the last
 *     L - 1 samples of earlier calls, zeros after create and after reset.  The scale multiplies the finished dot product, as
 *     firfilt_*_set_scale has it.
 *   Arithmetic: plain f32 without contraction, f32 subnormals kept.  Per output acc = +0; for i = 0, 1 .. L - 1 in that
 *     order acc = acc + h[i] * x[t - i], the product rounded, then the sum; y = s * acc, always multiplied, no tap skipped;
 *     complex samples: the same on re and im separately.  The result does not depend on the call size, on where a stream
 *     is cut, on nchan or on host versus device entry, bit for bit.
 *   csdr_firdes_kaiser (no GPU needed): liquid_firdes_kaiser(n, fc, As, 0): h[i] = sinc(2 fc t) w(i), t = i - (n - 1) / 2,
 *     w the Kaiser window of beta(As) with the argument 2 t / (n - 1); evaluated in f64 and rounded once (the form the
 *     known answers of images/ex1_5.gif pin).  CSDR_ERR_INVALID: n < 2, n > 2048, fc outside (0, 0.5], as_db <= 0,
 *     mu != 0 (every call in the reference passes 0), h NULL.
 *   csdr_fir_groupdelay (no GPU needed): Re(sum i h[i] e^{j 2 pi fc i} / sum h[i] e^{j 2 pi fc i}), accumulated in f32
 *     (liquid's fir_group_delay as recalled); CSDR_ERR_INVALID: NULL, n = 0, |fc| > 0.5.
 *   create_kaiser: the taps of csdr_firdes_kaiser and s = 2 fc, evaluated in f32.  create_taps: the caller's taps
 *     (copied) and scale; 1 <= n <= 2048 (this library's limit).  is_complex: 0 F32 rows, otherwise CF32 rows.
 *   process: x and y are [nchan][n]; any n <= max_samples (max_samples 0 means 4096), n = 0 is a no-op; x and y must not
 *     overlap.  n > max_samples: CSDR_ERR_SIZE; NULL or bad arguments: CSDR_ERR_INVALID; no GPU: CSDR_ERR_NODEV.
 * ------------------------------------------------------------------------ */
typedef struct csdr_firfilt csdr_firfilt;
int csdr_firdes_kaiser(uint32_t n, float fc, float as_db, float mu, float *h);
int csdr_fir_groupdelay(const float *h, uint32_t n, float fc, float *gd);
int csdr_firfilt_create_kaiser(uint32_t n, float fc, float as_db, float mu, int32_t is_complex, uint32_t nchan,
                               uint32_t max_samples, csdr_firfilt **out);
int csdr_firfilt_create_taps(const float *h, uint32_t n, float scale, int32_t is_complex, uint32_t nchan,
                             uint32_t max_samples, csdr_firfilt **out);
int csdr_firfilt_process(csdr_firfilt *h, const float *x, uint32_t n, float *y);
/* device buffers as above; enqueued on `stream`, no synchronisation */
int csdr_firfilt_process_device(csdr_firfilt *h, const void *d_x, uint32_t n, void *d_y, void *stream);
int csdr_firfilt_reset(csdr_firfilt *h);                          /* the history back to zeros                       */
uint32_t csdr_firfilt_get_taps_len(const csdr_firfilt *h);
int csdr_firfilt_get_taps(const csdr_firfilt *h, float *taps, float *scale);   /* either pointer may be NULL        */
int csdr_firfilt_destroy(csdr_firfilt *h);

/* ------------------------------------------------------------------------ *
 * gmskDemodulator m k bw  (Liquid.chs:384-429), `nchan` independent CF32 streams: GMSK with k samples per symbol, a filter
 * delay of m symbols and the bandwidth-time product BT.  Replaces gmskdem_create(k, m, BT) / gmskdem_demodulate per symbol /
 * gmskdem_destroy (imports :386-396).  The argument order (k, m, bt) is liquid's; the Haskell gmskDemodulator m k bw hands
 * `k m bw` on (:409).  liquid-dsp 1.3.2's gmskdem as recalled (unpinned) around a receive filter that is this library's own
 * and pinned by its definition.
 *   The two designs (no GPU needed), L = 2 k m + 1 taps each, evaluated in f64 and rounded once:
 *     csdr_firdes_gmsktx: the Gaussian-filtered rectangular frequency pulse.  t_i = i / k - m, c = 2 pi BT / sqrt(ln 2),
 *       g~_i = Q(c (t_i - 1/2)) - Q(c (t_i + 1/2)), Q(x) = erfc(x / sqrt 2) / 2, g = g~ / sum g~: the taps sum to one
 *       (liquid scales them to pi / 2 k; that factor is the modulator's here).
 *     csdr_firdes_gmskrx: NOT liquid_firdes_gmskrx.  The r of least sum r^2 whose cascade with g has no inter-symbol
 *       interference over its own span: c = g * r (full convolution, centre L - 1), c[L - 1] = 1, c[L - 1 + j k] = 0 for
 *       0 < |j| <= m.  With A[j + m][i] = g[L - 1 + j k - i] (0 outside [0, L)), g the f64 pulse: (A A^T) lambda = e_m by
 *       Gaussian elimination with partial pivoting, r = A^T lambda, r_i <- (r_i + r_{L-1-i}) / 2, then rounded: the f32 taps
 *       are exactly symmetric.
 *     CSDR_ERR_INVALID: k outside [2, 64], m outside [1, 8], BT outside [0.2, 1] (this library's limits: below 0.2 the
 *       system degenerates), h NULL.
 *   demodulator: phi[t] = arg(conj(x[t - 1]) x[t]) as every freqdem of this library computes it (kf = 1 / 2 pi: radians);
 *     x[t < 0] is the row's history: the last L samples of earlier calls, zeros after create and after reset.  Symbol s of a
 *     call covers the samples s k .. s k + k - 1; its soft value is d[s] = sum_{i < L} r[i] phi[s k - i], the filter output
 *     after the symbol's first sample has been pushed, as liquid has it; sym[s] = d[s] > 0 ? 1 : 0.
 *   Arithmetic: plain f32 without contraction; acc = +0; for i = 0, 1 .. L - 1 in that order acc = acc + r[i] * phi[s k - i],
 *     the product rounded, then the sum.  The result does not depend on the call size, on nchan, on whether soft is asked
 *     for or on host versus device entry, bit for bit.
 *   process: x is [nchan][n] CF32; sym is [nchan][n / k] uint32; soft, when not NULL, is [nchan][n / k] F32; *n_out =
 *     nchan * (n / k).  n must be a multiple of k (the reference throws, :421): otherwise CSDR_ERR_SIZE with the state
 *     untouched; n > max_samples: CSDR_ERR_SIZE (max_samples 0 means 4096); n = 0 is a no-op; NULL: CSDR_ERR_INVALID.
 * ------------------------------------------------------------------------ */
typedef struct csdr_gmskdem csdr_gmskdem;
int csdr_firdes_gmsktx(uint32_t k, uint32_t m, float bt, float *h);
int csdr_firdes_gmskrx(uint32_t k, uint32_t m, float bt, float *h);
int csdr_gmskdem_create(uint32_t k, uint32_t m, float bt, uint32_t nchan, uint32_t max_samples, csdr_gmskdem **out);
int csdr_gmskdem_process(csdr_gmskdem *h, const float *x_cf32, uint32_t n, uint32_t *sym, float *soft, uint32_t *n_out);
/* device buffers as above; d_soft may be NULL; enqueued on `stream`, no synchronisation */
int csdr_gmskdem_process_device(csdr_gmskdem *h, const void *d_x, uint32_t n, void *d_sym, void *d_soft, void *stream);
int csdr_gmskdem_reset(csdr_gmskdem *h);                          /* the history back to zeros                       */
int csdr_gmskdem_get_design(const csdr_gmskdem *h, uint32_t *taps_len, float *taps);   /* either may be NULL         */
int csdr_gmskdem_destroy(csdr_gmskdem *h);

/* ------------------------------------------------------------------------ *
 * iirCFilter n fc f0 ap as  (Liquid.chs:594-608) = iirfilt_crcf_create_prototype(BUTTER, LOWPASS, SOS, n, fc, f0, ap, as),
 * its real-valued form for any order, and the same object made from the caller's own sections: a cascade of S second-order
 * sections (1 <= S <= 8) with real coefficients on `nchan` independent rows of F32 or CF32 samples.  csdr_iirfilt_* above
 * (one order-2 section, F32) is unchanged.
 *   section s: b[3 s .. 3 s + 2], a[3 s .. 3 s + 2] with a0 = 1.  Per sample, direct form II as in csdr_iirfilt:
 *       v0 = x - a1 v1 - a2 v2;  y = b0 v0 + b1 v1 + b2 v2;  (v1, v2) <- (v0, v1)
 *     The sections run in order s = 0 .. S - 1, each on the output of the one before.  On CF32 rows the real and the imaginary
 *     part are filtered alike (iirfilt_crcf).  (v1, v2) of every section and row is zero after create and after reset and is
 *     carried from call to call.  The result follows the sequential f32 loop up to summation order: the row is evaluated as a
 *     blocked scan (4096 samples per block, block states combined in f64), so it is not bit-identical to that loop, nor between
 *     two ways of cutting one stream into calls.  A row is one workgroup's work: nchan = 1 runs on one compute unit.
 *   csdr_iirdes_butter_lowpass (no GPU needed): Butterworth low-pass of order n, 1 <= n <= 16, cut-off fc in (0, 0.5) cycles per
 *     sample, S = ceil(n / 2) sections into b[3 S], a[3 S].  Analog poles exp(+-j theta_i), theta_i = (2 (i + 1) + n - 1) pi /
 *     (2 n) for i < floor(n / 2), and -1 for odd n; bilinear transform with pre-warping m = tan(pi fc): p_d = (1 + m p) /
 *     (1 - m p), all zeros at -1.  One section per conjugate pair in the order i = 0, 1, .. (highest Q first): a = [1, -2 Re p_d,
 *     |p_d|^2], b = g [1, 2, 1]; for odd n a first-order section last: a = [1, -p_d, 0], b = g [1, 1, 0].  g gives every
 *     section unit DC gain (liquid spreads the overall gain over the sections in equal parts: the product is the same).
 *     Evaluated in f64 and rounded once.  For n = 2 these are csdr_iirfilt's coefficients.
 *   create_prototype: that design; f0, ap and as_db do not enter a Butterworth low-pass and are ignored, as in
 *     csdr_iirfilt_create.  create_sos: the caller's nsec sections (copied), each divided by its a0 (iirfiltsos).
 *     is_complex: 0 F32 rows, otherwise CF32 rows.
 *   process: x and y are [nchan][n]; any n <= max_samples (max_samples 0 means 4096), n = 0 is a no-op.  process_device: x and y
 *     may be the same buffer, but must not overlap otherwise.
 *   CSDR_ERR_INVALID: order 0 or > 16, fc <= 0 or >= 0.5, nsec 0 or > 8, a section with a0 = 0 or one that is not strictly
 *     stable (needs |a2| < 1 and |a1| < 1 + a2 after the division), nchan 0, NULL arguments; n > max_samples: CSDR_ERR_SIZE;
 *     no GPU: CSDR_ERR_NODEV.
 * ------------------------------------------------------------------------ */
typedef struct csdr_iirsos csdr_iirsos;
int csdr_iirdes_butter_lowpass(uint32_t order, float fc, float *b, float *a);
int csdr_iirsos_create_prototype(uint32_t order, float fc, float f0, float ap, float as_db, int32_t is_complex, uint32_t nchan,
                                 uint32_t max_samples, csdr_iirsos **out);
int csdr_iirsos_create_sos(const float *b, const float *a, uint32_t nsec, int32_t is_complex, uint32_t nchan,
                           uint32_t max_samples, csdr_iirsos **out);
int csdr_iirsos_process(csdr_iirsos *h, const float *x, uint32_t n, float *y);
/* device buffers as above; enqueued on `stream`, no synchronisation.  d_y may be d_x itself (in place) or must not overlap
 * it.  The launch goes to the calling thread's current device, which has to be the one the handle was created on */
int csdr_iirsos_process_device(csdr_iirsos *h, const void *d_x, uint32_t n, void *d_y, void *stream);
int csdr_iirsos_reset(csdr_iirsos *h);                            /* every section's state back to zero              */
uint32_t csdr_iirsos_get_nsec(const csdr_iirsos *h);
int csdr_iirsos_get_sos(const csdr_iirsos *h, float *b, float *a);   /* [3 nsec] each, a0 = 1; either may be NULL      */
int csdr_iirsos_destroy(csdr_iirsos *h);

/* ------------------------------------------------------------------------ *
 * firpfbch2Channelizer M m as: liquid's 2x-oversampled polyphase channelizer, firpfbch2_crcf, as an analyzer.  The reference
 * itself does NOT import it (Liquid.chs binds only firpfbch_crcf, :813-866); the block stands for what a Haskell binding of
 * firpfbch2_crcf_create_kaiser / _create / _execute (analyzer) / _reset / _destroy would call.  Recalled from liquid-dsp
 * 1.3.2, unpinned.
 *   M channels, a power of two in [4, 256]; prototype semi-length m in [1, 8]; a real prototype h[0 .. L - 1], L = 2 m M.
 *   A call takes n samples, a multiple of M / 2, and yields frames = n / (M / 2) output frames, channel-major: y[k][t], M rows
 *   of `frames` CF32 samples.  With t counting frames from the start of the stream and n_t = (t + 1) M / 2 - 1,
 *     y_k[t] = (1 / M) sum_{i < L} h[i] x[n_t - i] e^{+j 2 pi k (i + t M / 2) / M},   x[s < 0] = 0:
 *   row k is a phase-continuous down-conversion by 2 pi k / M rad/sample (no pre-shift), low-passed by h, decimated by M / 2.
 *   The last L - M / 2 samples and the frame parity are carried from call to call.
 *   Arithmetic: f32.  v[i] = sum_n h[i + n M] x[n_t - i - n M] by fmaf from +0, oldest sample first; the DFT input is rotated
 *     by M / 2 on odd frames; an M-point backward radix-2 DFT (a complex product is one product and one fma per component)
 *     whose operation order depends on M only; the scale 1 / M is exact.  The output is bit-identical for every chunking of
 *     the stream and for host versus device entry.
 *   csdr_pfbch2_design (no GPU needed): 2 M m + 1 taps of liquid_firdes_kaiser(., fc, as_db, 0) (csdr_firdes_kaiser's form),
 *     fc = 0 meaning the recalled rule for an analyzer, fc = 1 / M; f64, scaled so that all 2 M m + 1 sum to M, rounded once;
 *     the first 2 M m are returned and used, as firpfbch drops the last.
 *   csdr_pfbch2_launch_shape (no GPU needed): how a call of `frames` frames runs on a device of `cus` compute units:
 *     shape[6] = frames per tile, tiles, consecutive tiles per workgroup, workgroups, workgroups per CU, LDS bytes per workgroup.
 *   open_kaiser = the design, then open_taps (firpfbch2_crcf_create_kaiser / _create); rewind is firpfbch2_crcf_reset: the
 *     state right after open.  (`open` / `rewind`, not `create` / `reset`: the names of this block only.)
 *   CSDR_ERR_INVALID: M not a power of two in [4, 256], m outside [1, 8], as_db <= 0 or not finite, fc < 0 or >= 0.5 or not
 *     finite, max_frames = 0 or max_frames M > 2^31, NULL, a non-finite tap, x and y the same buffer.  CSDR_ERR_SIZE: n not a
 *     multiple of M / 2, or more than max_frames frames; the state is untouched.  No GPU: CSDR_ERR_NODEV.
 * ------------------------------------------------------------------------ */
typedef struct csdr_pfbch2 csdr_pfbch2;
int csdr_pfbch2_design(uint32_t M, uint32_t m, float as_db, float fc, float *h /* [2 M m] */);
int csdr_pfbch2_launch_shape(uint32_t M, uint32_t m, uint32_t frames, uint32_t cus, uint32_t *shape /* [6] */);
int csdr_pfbch2_open_kaiser(uint32_t M, uint32_t m, float as_db, float fc, uint32_t max_frames, csdr_pfbch2 **out);
int csdr_pfbch2_open_taps(const float *h /* [2 M m] */, uint32_t M, uint32_t m, uint32_t max_frames, csdr_pfbch2 **out);
int csdr_pfbch2_process(csdr_pfbch2 *h, const float *x_cf32, uint32_t n, float *y_cf32 /* [M][2 n / M] */, uint32_t *frames);
/* device buffers as above; enqueued on `stream`, no synchronisation */
int csdr_pfbch2_process_device(csdr_pfbch2 *h, const void *d_x, uint32_t n, void *d_y, void *stream);
int csdr_pfbch2_rewind(csdr_pfbch2 *h);                           /* back to the state right after open               */
int csdr_pfbch2_get_taps(const csdr_pfbch2 *h, float *taps /* [2 M m] */);
int csdr_pfbch2_destroy(csdr_pfbch2 *h);

/* ------------------------------------------------------------------------ *
 * firpfbch2Synthesizer M m as: the synthesizer side of liquid's firpfbch2_crcf, the way back from csdr_pfbch2's rows to one
 * stream (channelize, work on or drop rows, re-assemble).  Not imported by the reference either.
 *   Recalled from liquid-dsp 1.3.2, unpinned by liquid: the structure (an M-point backward DFT per frame, M / 2 outputs per
 *     frame from alternating halves of the last 4 m transforms) and the design rule, a cutoff of 0.5 / M, half the analyzer's.
 *   This library's own: the scale.  liquid's is not recalled; the factor 1/2 below makes analysis followed by synthesis unit-gain.
 *   What pins both halves without liquid: with the analyzer's prototype cut at 1 / M and this one's at 0.5 / M,
 *     csdr_pfbch2 followed by csdr_pfbsyn2 returns its input delayed by D = 2 M m - M / 2 + 1 samples (liquid's figure): rel-RMS
 *     4.3e-5 and gain 1.00002 at m = 7, 80 dB in f64; with equal cutoffs on both sides the rel-RMS is above 0.15.  The pair of
 *     cutoffs is pinned, not which side has which: exchanged, they return the input as well.
 *   M, m as csdr_pfbch2's; a real prototype g[0 .. L - 1], L = 2 m M; P = M / 2.  A call takes `frames` frames, channel-major as
 *   csdr_pfbch2 writes them, Y[k][t] with the row stride `frames`, and yields frames P samples.  With t counting frames from
 *   the start of the stream, w_t[q] = sum_{k < M} Y_k[t] e^{+j 2 pi k q / M} and r < P,
 *     x[t P + r] = 1/2 sum_{n = 0 .. 4 m - 1, t - n >= 0} g[r + n P] w_{t-n}[(r + t P) mod M]
 *   ( = 1/2 sum_t g[s - t P] sum_k Y_k[t] e^{+j 2 pi k s / M}).  The last 4 m - 1 input frames, how many of them belong to the
 *   stream, and the frame parity are carried from call to call.
 *   Arithmetic: f32.  The DFT is radix-2 (a complex product is one product and one fma per component) in an order that depends on
 *     M only; the sum over n by fmaf from +0, oldest frame first, frames in front of the stream skipped; the factor 1/2 is exact.
 *     The output is bit-identical for every chunking of the stream and for host versus device entry.
 *   csdr_pfbsyn2_design (no GPU needed): csdr_pfbch2_design's Kaiser design with fc = 0 meaning 0.5 / M.
 *   csdr_pfbsyn2_launch_shape (no GPU needed): as csdr_pfbch2_launch_shape, for this block's kernel.
 *   open_kaiser / open_taps / rewind as csdr_pfbch2's.  csdr_pfbsyn2_delay: D above (0 for NULL).
 *   CSDR_ERR_INVALID: as csdr_pfbch2's (bad M, m, as_db, fc, max_frames, NULL, a non-finite tap, y and x the same buffer).
 *     CSDR_ERR_SIZE: more than max_frames frames; the state is untouched.  No GPU: CSDR_ERR_NODEV.  0 frames: a no-op.
 * ------------------------------------------------------------------------ */
typedef struct csdr_pfbsyn2 csdr_pfbsyn2;
int csdr_pfbsyn2_design(uint32_t M, uint32_t m, float as_db, float fc, float *g /* [2 M m] */);
int csdr_pfbsyn2_launch_shape(uint32_t M, uint32_t m, uint32_t frames, uint32_t cus, uint32_t *shape /* [6] */);
int csdr_pfbsyn2_open_kaiser(uint32_t M, uint32_t m, float as_db, float fc, uint32_t max_frames, csdr_pfbsyn2 **out);
int csdr_pfbsyn2_open_taps(const float *g /* [2 M m] */, uint32_t M, uint32_t m, uint32_t max_frames, csdr_pfbsyn2 **out);
int csdr_pfbsyn2_process(csdr_pfbsyn2 *h, const float *y_cf32 /* [M][frames] */, uint32_t frames, float *x_cf32 /* [frames M / 2] */, uint32_t *n);
/* device buffers as above; enqueued on `stream`, no synchronisation */
int csdr_pfbsyn2_process_device(csdr_pfbsyn2 *h, const void *d_y, uint32_t frames, void *d_x, void *stream);
int csdr_pfbsyn2_rewind(csdr_pfbsyn2 *h);                         /* back to the state right after open               */
int csdr_pfbsyn2_get_taps(const csdr_pfbsyn2 *h, float *taps /* [2 M m] */);
uint32_t csdr_pfbsyn2_delay(const csdr_pfbsyn2 *h);               /* 2 M m - M / 2 + 1 samples through both banks     */
int csdr_pfbsyn2_destroy(csdr_pfbsyn2 *h);

/* ------------------------------------------------------------------------ *
 * rowResampler rate m as fc: liquid's resamp_crcf / resamp_rrrf (an arbitrary-rate polyphase resampler) on nchan rows at once,
 * all CF32 or all F32, behind csdr_pfbch / csdr_pfbch2 and in front of the blocks that want a whole number of samples per
 * symbol or a fixed audio rate.  The reference imports neither interface (its `resampler` is msresamp_crcf on one stream:
 * csdr_resamp_* above, which stays as it is).
 *   Own spec, "csdr rowresamp v1" (DESIGN.md 4.19), not liquid's bit for bit:
 *   Timing: delta = llround(2^32 / rate) is Q32.32 input samples per output, so the rate that runs is 2^32 / delta.  Output k of
 *     the stream sits at t_k = k delta: sample n_k = t_k >> 32, phase b = (t_k >> 24) & 255, mu = (t_k & 0xffffff) / 2^24.  The
 *     handle carries T, the time of the next output relative to the first sample of the next call (0 at open).  A call of n
 *     samples per row yields n_out = 0 if (T >> 32) >= n, else floor(((n << 32) - 1 - T) / delta) + 1 outputs per row, the same
 *     for every row; then T <- T + n_out delta - (n << 32).  Output k belongs to the call that delivers sample n_k.
 *   Filter: 256 phases, P = 2 m D taps per phase, D = 1 for delta <= 2^32, else ceil(delta / 2^32) ( = ceil(1 / r)); fc = 0 means
 *     min(0.515 min(r, 1), 0.49); g = liquid_firdes_kaiser(256 P + 1, fc / 256, as); bank[b][j] = f32(2 fc g[b + 256 j]) for
 *     b = 0 .. 256 (row 256 is row 0 one sample later).  s0 = sum_j bank[b][j] x[n_k - j], s1 the same with row b + 1,
 *     y_k = fma(mu, s1, (1 - mu) s0), re and im apart; x[s < 0] = 0.  Group delay: m D input samples.
 *   Arithmetic: f32; s0 and s1 by fmaf from +0 in the order j = 0 .. P - 1.  The output is bit-identical for every chunking of
 *     the stream, for a row alone against the same row among others, for host versus device entry and after rewind.
 *   Limits: 1/8 <= rate <= 8; 1 <= m <= 8 with m D <= 56; 0 < as_db <= 120; fc = 0 or 0 < fc < 0.5; nchan >= 1;
 *     1 <= max_samples <= 2^28 (samples per row and call).  Anything else: CSDR_ERR_INVALID.
 *   x is [nchan][n], y is [nchan][n_out], both dense; csdr_rowresamp_max_out(h, n) is the room per row a call of n may need
 *     and csdr_rowresamp_count(h, n) what the next call of n yields.  The count comes from integers on the host:
 *     process_device enqueues on `stream` and does not synchronise.
 *   csdr_rowresamp_design, csdr_rowresamp_launch_shape: no GPU needed.  shape = {P, outputs per tile, window slots, LDS bytes,
 *     workgroups per CU, tiles per row, items per run, runs}.
 *   CSDR_ERR_SIZE: more than max_samples samples.  NULL, x and y the same buffer: CSDR_ERR_INVALID.  A refused call leaves the
 *     stream untouched.  No GPU: CSDR_ERR_NODEV.  n = 0: yields nothing.  destroy(NULL) is 0.
 * ------------------------------------------------------------------------ */
typedef struct csdr_rowresamp csdr_rowresamp;
int csdr_rowresamp_design(double rate, uint32_t m, float as_db, float fc, uint32_t *taps_per_phase, uint64_t *delta,
                          float *bank /* [257][P] or NULL */);
int csdr_rowresamp_launch_shape(double rate, uint32_t m, int32_t is_complex, uint32_t n_out, uint32_t nchan, uint32_t cus,
                                uint64_t t_next, uint32_t *shape /* [8] */);
int csdr_rowresamp_open(double rate, uint32_t m, float as_db, float fc, int32_t is_complex, uint32_t nchan, uint32_t max_samples,
                        csdr_rowresamp **out);
uint32_t csdr_rowresamp_max_out(const csdr_rowresamp *h, uint32_t n);            /* room a caller provides per row          */
int csdr_rowresamp_count(const csdr_rowresamp *h, uint32_t n, uint32_t *n_out);  /* what the next call of n yields          */
int csdr_rowresamp_process(csdr_rowresamp *h, const float *x, uint32_t n, float *y, uint32_t *n_out);
int csdr_rowresamp_process_device(csdr_rowresamp *h, const void *d_x, uint32_t n, void *d_y, uint32_t *n_out, void *stream);
int csdr_rowresamp_rewind(csdr_rowresamp *h);                                    /* back to the state right after open      */
int csdr_rowresamp_get_design(const csdr_rowresamp *h, uint32_t *taps_per_phase, uint64_t *delta, uint32_t *delay,
                              float *bank);                                      /* any pointer may be NULL                 */
int csdr_rowresamp_get_time(const csdr_rowresamp *h, uint64_t *t_next);
int csdr_rowresamp_destroy(csdr_rowresamp *h);

/* ------------------------------------------------------------------------ *
 * pskTracker bits sps ..: what liquid's symtrack_cccf (symTracker m k, Liquid.chs:119-175) does behind its symbol
 * synchroniser, on `nchan` independent CF32 rows: power normaliser, carrier PLL, T/2-spaced equaliser, BPSK / QPSK decision.
 * symTracker m k is then csdr_symsync (k_out = 2, RRC 0.25) followed by this block with bits 1, sps 2, eq_len 9, constant
 * modulus.  Own spec, "csdr psktrack v1" (DESIGN.md 4.20), not liquid's bit for bit.  Per input sample v of a row, in this order:
 *   1. p += agc_bw (|v|^2 - p), p = 1 at start and kept >= 2^-100; v /= sqrt(p).  Deviation: liquid's agc_crcf (an exp / log
 *      recurrence that cannot be restated bit for bit) is replaced by this normaliser.
 *   2. v *= conj(e^(j theta)); theta += freq.  theta and freq are uint32 phase words, 2^32 = one turn; sine and cosine of a word
 *      are csdr_sincos_word below.
 *   3. With an equaliser v enters a window of eq_len samples.  At sps 2 an output is due at every second sample: when the
 *      sample under the window's centre tap (without an equaliser: v itself) is sample number `phase` modulo 2 of the row,
 *      counted from the row's first sample after new / restart; the count carries across calls of any size.  At an output
 *      d = sum_i conj(w[i]) buf[i], i = 0 (oldest) .. eq_len - 1, the weights starting as a unit centre tap; without an equaliser
 *      d = v.
 *   4. Decision.  BPSK: bit 0 = (d.re < 0), x_hat = +-1.  QPSK: bit 0 = (d.re < 0), bit 1 = (d.im < 0), x_hat = (+-1 +-j) / sqrt 2.
 *      The symbol number is those bits, a Gray code: 0 (+, +), 1 (-, +), 3 (-, -), 2 (+, -) around the circle.
 *   5. e = Im(d conj(x_hat)); freq += word(pll_bw e); theta += word(sqrt(pll_bw) e) (nco_pll_step with alpha = pll_bw,
 *      beta = sqrt(pll_bw)).  word(r) = r * f32(2^31 / pi), NaN -> 0, clamped to +-2^30, rounded to nearest (ties to even),
 *      added modulo 2^32.
 *   6. From output number eq_delay on: w[i] += eq_mu conj(err) buf[i] / (sum |buf|^2 + 2^-20), err = x_hat - d (decision-
 *      directed) or d / |d| - d (constant modulus; 0 when |d| = 0).
 *   7. y gets d, sym (unless NULL) the symbol number.
 *   Arithmetic: f32, nothing contracted, every sum in the order of kernels_psktrack.hip; / and sqrt correctly rounded.  The
 *     output is bit-identical for every chunking (odd sizes at sps 2 included), row count, row position and host versus device
 *     entry; tests/psktrack_restatement.py restates it.  The 180 / 90 degree ambiguity is the caller's to resolve.
 *   Rows have their own lengths: x is [nchan][n], nx[c] <= n the samples of row c (NULL: every row holds n); y and sym are
 *     [nchan][n] (row stride n), row c holding ny[c] outputs.  This is what csdr_symsync_process_c_device writes, so the two
 *     device entries chain on one stream with no synchronisation between.  On the device path a count above n is clamped to n.
 *   Limits: bits 1 | 2; sps 1 | 2; phase 0 | 1; eq_len 0, or odd in [3, 17] with sps 2; eq_mu, pll_bw, agc_bw in [0, 1];
 *     nchan >= 1; max_samples <= 2^28.  Anything else: CSDR_ERR_INVALID, before a device is looked for.  No GPU: CSDR_ERR_NODEV.
 *   CSDR_ERR_SIZE: n > max_samples, or (host path) nx[c] > n.  A refused call leaves the rows untouched.  destroy(NULL) is 0,
 *     restart(NULL) CSDR_ERR_INVALID.
 * ------------------------------------------------------------------------ */
#define CSDR_PSKTRACK_EQ_DD 0u           /* eq_mode: decision-directed                                      */
#define CSDR_PSKTRACK_EQ_CM 1u           /* eq_mode: constant modulus                                       */
#define CSDR_PSKTRACK_EQ_MU 0.05f        /* the defaults that the Pipes pass                                */
#define CSDR_PSKTRACK_EQ_DELAY 200u      /* liquid's symtrack                                               */
#define CSDR_PSKTRACK_PLL_BW 9e-4f       /* liquid's symtrack default bandwidth 0.001 x 0.9, as recalled    */
#define CSDR_PSKTRACK_AGC_BW 0.02f
typedef struct csdr_psktrack csdr_psktrack;
/* (sin, cos) of a phase word, as the kernel computes them: octant from the top 3 bits, the 29-bit remainder (reflected in odd
 * octants) times f32(pi 2^-31), then sin a = ((((S3 z + S2) z + S1) z) a) + a and cos a = (1 - 0.5 z) + ((((C3 z + C2) z + C1) z) z)
 * with z = a a, in f32, each operation rounded (coefficients: psktrack_common.h).  |error| <= 2^-21.  No GPU needed */
int csdr_sincos_word(uint32_t w, float *s, float *c);
int csdr_psktrack_new(uint32_t bits, uint32_t sps, uint32_t phase, uint32_t eq_len, float eq_mu, uint32_t eq_mode, uint32_t eq_delay,
                      float pll_bw, float agc_bw, uint32_t nchan, uint32_t max_samples, csdr_psktrack **out);
int csdr_psktrack_process(csdr_psktrack *h, const float *x /* CF32 [nchan][n] */, uint32_t n, const uint32_t *nx /* [nchan] or NULL */,
                          float *y /* CF32 [nchan][n] */, uint32_t *sym /* [nchan][n] or NULL */, uint32_t *ny /* [nchan] */);
/* device buffers as above (d_nx, d_sym may be NULL); enqueued on `stream`, no synchronisation */
int csdr_psktrack_process_device(csdr_psktrack *h, const void *d_x, uint32_t n, const void *d_nx, void *d_y, void *d_sym, void *d_ny,
                                 void *stream);
int csdr_psktrack_restart(csdr_psktrack *h);                      /* back to the state right after new                */
/* row chan: phase and frequency words, power estimate, outputs so far (saturating), weights [eq_len] CF32; any may be NULL */
int csdr_psktrack_get_state(csdr_psktrack *h, uint32_t chan, uint32_t *theta, uint32_t *freq, float *p, uint32_t *nsym, float *w);
/* alpha = pll_bw and beta = sqrt(pll_bw) as f32, eq_len, the kernel's LDS bytes per workgroup; any may be NULL */
int csdr_psktrack_get_design(const csdr_psktrack *h, float *alpha, float *beta, uint32_t *eq_len, uint32_t *lds_bytes);
int csdr_psktrack_destroy(csdr_psktrack *h);

/* ------------------------------------------------------------------------ *
 * The fused chain: everything assembleFold (apps/SoapySDR.hs:208-226) puts
 * behind `compact`:
 *     dcBlocker                                   (SoapySDR.hs:213-214)
 *  -> firpfbchChannelizer M  = NCO pre-mix + firpfbch_crcf analyzer +
 *     transpose to channel-major                  (Liquid.chs:811-866)
 *  -> per channel: [automaticGainControl] -> [fmDemodulator kf]
 *                                                 (SoapySDR.hs:190-199, 249)
 *  -> [mix]                                       (Trans.hs:119-122)
 * replacing  mix . mux (replicate nch demod) . firpfbchChannelizer nc  and
 * firpfbchChannelizer nc + distribute_ (addPipe demod sink)  (SoapySDR.hs:218-225).
 * For channels == 1 it is  demod  alone behind the DC blocker (SoapySDR.hs:226).
 *
 * process(): in = n_in CF32 samples, n_in a multiple of `channels`
 *   (the reference's chunk is 4*channels*1024, SoapySDR.hs:215; the reference
 *   misbehaves for other remainders, SURVEY.md a6 -> CSDR_ERR_SIZE here).
 *   out = ONE contiguous channel-major buffer [chan_count][nf], nf = n_in/channels,
 *   element CF32 (demod none) or F32 (FM); with mix: [nf] only.  The caller
 *   slices it into per-channel arrays exactly like Liquid.chs:850-862.
 *   *n_out = number of output ELEMENTS written.  n_in == 0 is a no-op.
 * ------------------------------------------------------------------------ */
typedef struct csdr_chain csdr_chain;

typedef struct csdr_chain_cfg {
    uint32_t struct_size;       /* = sizeof(csdr_chain_cfg)                              */
    uint32_t channels;          /* -c M, >= 1                                            */
    uint32_t dc_block;          /* 1: include dcBlocker (assembleFold always does)       */
    float    dc_alpha;          /* 0.0005 (Liquid.chs:577); in (0, 1) with dc_block, else CSDR_ERR_INVALID.
                                 * The fused kernels and k_dc_tile cut the DC state after fixed windows sized for 0.0005:
                                 * alpha < 0.0005 or > ~0.15 (whose fold weights beta^-512 overflow f32) runs the any-M
                                 * route with the exact block scan instead (path "...+dc-scan")         */
    float    agc_threshold_db;  /* -a tres; 0 = no AGC (SoapySDR.hs:195-198)             */
    uint32_t demod;             /* CSDR_DEMOD_*                                          */
    float    kf;                /* DeNBFM kf                                             */
    uint32_t mix;               /* --mix                                                 */
    uint32_t chan_first;        /* channel shard [chan_first, chan_first+chan_count)     */
    uint32_t chan_count;        /*   0 = all channels                                    */
    int32_t  device;            /* HIP device ordinal, -1 = current device               */
    uint32_t max_frames;        /* largest n_in/channels per call; 0 = 4096              */
    uint32_t flags;             /* CSDR_FLAG_*                                           */
    uint32_t pfb_m;             /* filter semi-length m, 0 = 7  (Liquid.chs:813); 1..32, else CSDR_ERR_INVALID.
                                 * Fused kernels exist for m = 7 only (other m: the any-M route); the DeNo --mix
                                 * identity folds need 2m <= 33                                                   */
    float    pfb_as;            /* stop-band attenuation, 0 = 80 dB (Liquid.chs:813)     */
    uint32_t wbfm_decim;        /* DeWBFM decim (SoapySDR.hs:252-259); 0 = 4             */
    float    deemph_fc;         /* DeWBFM de-emphasis corner 5000/quadRate (Liquid.chs:655); 0 = 0.025 */
    uint32_t chan_stride;       /* G > 1: interleaved channel ownership for channel-sharded multi-GPU runs
                                 * (SURVEY 8e(A)): this handle produces the channels chan_first, chan_first + G, ...
                                 * (chan_first < G, G divides channels, chan_count 0 or channels/G); output row m is
                                 * channel chan_first + G*m.  channels = 256 or 1024 with G = 2, 4, 8: the fused run kernels'
                                 * shard variants (the shift by chan_first rides on the pre-mix phasors, the DFT passes and
                                 * the freqdem / stores run for the owned channels only); every other shape: the M-point DFT
                                 * of a frame is pruned to one length-G fold plus one (channels/G)-point DFT on the any-M
                                 * route.  Either way a shard does 1/G of the DFT and tail work, while DC blocker, pre-mix
                                 * and FIR still see every branch.  0 / 1 = contiguous shard. */
} csdr_chain_cfg;

void csdr_chain_cfg_default(csdr_chain_cfg *cfg, uint32_t channels);
int  csdr_chain_create(const csdr_chain_cfg *cfg, csdr_chain **out);
int  csdr_chain_process(csdr_chain *h, const float *in_cf32, uint32_t n_in, void *out, uint32_t *n_out);
int  csdr_chain_process_device(csdr_chain *h, const void *d_in_cf32, uint32_t n_in,
                               void *d_out, uint32_t *n_out, void *stream);
/* Asynchronous host-buffer entry point (what a streaming caller such as the reference's fold uses; replaces the blocking
 * firpfbch/analyzer call at Liquid.chs:845 and the caller-owned buffers of Liquid.chs:82, :292): up to
 * CSDR_CHAIN_INFLIGHT chunks are in flight, H2D copy, kernels and D2H copy run on three streams so that the copies of
 * neighbouring chunks overlap the kernels.  `submit` returns as soon as the work is queued (CSDR_ERR_BUSY when
 * CSDR_CHAIN_INFLIGHT chunks are already pending); `collect` waits for the OLDEST submitted chunk, whose result is then
 * in the `out` given to its submit.  Buffers from csdr_host_alloc (page-locked) are copied from / to directly; any
 * other buffer is staged through page-locked memory owned by the handle (one extra host memcpy each way).  The
 * buffers of a chunk must stay valid until its collect.  csdr_chain_process = submit + collect. */
/* Pipelined DEVICE entry point, for callers that keep several chunks in flight in HBM (a capture ring, the bench): like
 * csdr_chain_process_device, but the work goes onto two handle-owned streams used alternately, and the call does not order
 * itself behind the previous chunk where the path allows it.  For the fused 256-channel chain without AGC / AM / WBFM
 * tails and chunks of whole 16-frame tiles at the run-kernel size, consecutive launches are INDEPENDENT: run 0 of a
 * chunk starts cold like every other run of the launch (DC state from a read-only warm-up over the previous chunk's last
 * tiles, which the handle keeps a copy of; FIR window and freqdem history from its last tile), so the next launch's
 * workgroups fill the compute units the previous launch has already left, and its cold start (tens of microseconds of
 * memory traffic with idle ALUs) runs under the previous launch's tile loops.  Same results as csdr_chain_process_device
 * to the run-start tolerance every run of a launch already has (DC state truncated at beta^24576).  Other configurations
 * are accepted and run serialized.
 *   ready_event: hipEvent_t after which d_in is complete, or NULL if it already is when the call is made.
 *   d_in must stay untouched and d_out unread until csdr_chain_wait_device (stream = NULL: the host waits for every
 *   submitted chunk; else `stream` is made to wait).  csdr_chain_process_device orders itself behind submitted chunks.
 * Stream lifetime: the handle never keeps a caller's `stream`; it records an event of its own behind the call's work, so a
 * caller stream may be destroyed once the caller itself has no further use for it (its pending work still completes). */
int  csdr_chain_submit_device(csdr_chain *h, const void *d_in_cf32, uint32_t n_in, void *d_out, uint32_t *n_out, void *ready_event);
int  csdr_chain_wait_device(csdr_chain *h, void *stream);
uint32_t csdr_chain_debug_independent_launches(const csdr_chain *h);   /* submit_device calls since create that ran as independent launches */
#define CSDR_CHAIN_INFLIGHT 3
void *csdr_host_alloc(size_t bytes);            /* page-locked host memory (hipHostMalloc); NULL on failure */
void  csdr_host_free(void *p);
int  csdr_chain_submit(csdr_chain *h, const float *in_cf32, uint32_t n_in, void *out);
int  csdr_chain_collect(csdr_chain *h, uint32_t *n_out);
/* Device-side health of the handle since the last check: CSDR_ERR_HIP (text in csdr_last_error) when an
 * inter-workgroup wait of the small-chunk kernels hit its spin limit (their output is then invalid), CSDR_OK
 * otherwise.  Synchronises the device; csdr_chain_process and csdr_chain_reset call it themselves, callers of the
 * device / async entry points call it at their own sync points. */
int  csdr_chain_status(csdr_chain *h);
int  csdr_chain_reset(csdr_chain *h);      /* back to the state right after create        */
/* Reset, then place the stream position at frame `frames` (n = frames*channels samples in):
 * the NCO pre-mix phase becomes what it would be there.  Used by time-striped multi-GPU runs,
 * where a rank starts in the middle of the stream behind a warm-up prefix. */
int  csdr_chain_seek_frames(csdr_chain *h, uint64_t frames);
int  csdr_chain_destroy(csdr_chain *h);

/* introspection used by the tests (mirrors what firpfbch_crcf_print / nco_crcf_print
 * show at Liquid.chs:814-820) */
uint32_t csdr_chain_out_elem_size(const csdr_chain *h);            /* 8 or 4 bytes        */
int  csdr_chain_get_taps(const csdr_chain *h, float *taps, uint32_t n); /* first M*2m taps */
int  csdr_chain_get_nco(const csdr_chain *h, uint32_t *theta, uint32_t *d_theta);
const char *csdr_chain_path(const csdr_chain *h);                  /* "fused-..." | "generic" */
/* The library's route table as text: which plan and which kernels a configuration (channels x chan_stride x output x AGC) gets,
 * per call shape.  csdr_chain_create selects from exactly this table. */
const char *csdr_route_table(void);
/* CSDR_FLAG_TIME_KERNELS: accumulated duration of the dominant kernel's launches
 * since the last call (synchronises the stream).  Returns the kernel's name. */
const char *csdr_chain_kernel_time(csdr_chain *h, double *total_ms, uint32_t *launches);

/* Diagnostics: with CSDR_TRACE=1 in the environment at create time the fused kernel records 16
 * s_memtime stamps per 16-frame tile; copies the stamps of the first `ntiles` tiles of the last
 * launch into out[ntiles][16] and returns the number of tiles copied (0 when tracing is off). */
int  csdr_chain_debug_trace(csdr_chain *h, unsigned long long *out, uint32_t ntiles);
/* Diagnostics of the time-parallel AGC tail since create: segments whose speculative start state was
 * checked against the true state, and how many of them had to be recomputed sequentially. */
int  csdr_chain_debug_agc(csdr_chain *h, uint32_t *checked, uint32_t *redone);
/* Calls since create whose AGC tail ran on a tile-major plane (k_agc_spec_tm: fused 256- and 1024-channel chains, run-sized calls of whole
 * 16-frame tiles; every other call takes the row-major k_agc_spec).  Both produce the sequential recurrence bit for bit. */
uint32_t csdr_chain_debug_agc_tile_major_calls(const csdr_chain *h);

/* the configuration a handle was created with (defaults filled in) */
int  csdr_chain_get_cfg(const csdr_chain *h, csdr_chain_cfg *cfg_out);

/* ------------------------------------------------------------------------ *
 * Collectives: one process per GPU, RCCL over xGMI (csrc/comm.cpp).
 *
 * The reference reduces `--mix` on one host thread: `mix` = foldl1 (+) over the channel
 * list (Trans.hs:119-122) behind `mux (replicate nch demod) . firpfbchChannelizer nc`
 * (SoapySDR.hs:217-222).  When the -c N channels are split over the GPUs of a node every
 * rank's chain folds its own channels and ONE all-reduce(SUM) of the nf output elements per
 * chunk adds the partial mixes (summation order differs from the strict left fold: tolerance).
 * Bootstrapping follows RCCL: rank 0 makes an id (csdr_comm_unique_id), the host hands the
 * CSDR_COMM_ID_BYTES to every rank by its own means (a file, an environment variable, the
 * Haskell program's command line), every rank calls csdr_comm_create with it (collective,
 * blocking).  librccl.so.1 is loaded on the first csdr_comm_* call, not with the library.
 * All calls enqueue on the caller's `stream` and do not synchronise.
 * ------------------------------------------------------------------------ */
#define CSDR_COMM_ID_BYTES 128
typedef struct csdr_comm csdr_comm;
int csdr_comm_unique_id(void *id_out);
int csdr_comm_create(int rank, int world, const void *id, int device /* -1 = current */, csdr_comm **out);
int csdr_comm_rank(const csdr_comm *c);
int csdr_comm_world(const csdr_comm *c);
int csdr_comm_destroy(csdr_comm *c);
/* d_buf (bytes) of rank `root` -> every rank: the chunk a channel-sharded node works on (8 B per input sample) */
int csdr_comm_broadcast(csdr_comm *c, void *d_buf, size_t bytes, int root, void *stream);
/* in-place sum over ranks of `count` floats */
int csdr_comm_allreduce_f32(csdr_comm *c, void *d_buf, size_t count, void *stream);
/* csdr_chain_process_device of a channel-shard handle created with mix = 1, then the all-reduce of its output: d_out holds
 * the mix over ALL channels on every rank (Trans.hs:119-122 across ranks).  *n_out = elements (nf). */
int csdr_chain_process_device_mix(csdr_chain *h, csdr_comm *c, const void *d_in_cf32, uint32_t n_in, void *d_out, uint32_t *n_out,
                                  void *stream);
/* The same for host buffers (blocking, like csdr_chain_process): what a host that keeps its chunks in its own memory calls --
 * the Haskell fold, host/soapy_sdr_file.cpp --world/--rank.  Every rank receives the full mix; the reference has ONE sink for it
 * (SoapySDR.hs:217-222), so rank 0 writes the file. */
int csdr_chain_process_mix(csdr_chain *h, csdr_comm *c, const float *in_cf32, uint32_t n_in, void *out, uint32_t *n_out);
/* The exchange of the hybrid partition (replaces the hand-over between firpfbchChannelizer and `mux`, Trans.hs:124-129,
 * when time stripes feed channel-block tails): d_plane = this rank's front-end output [world][chan_per_rank][stripe_frames[rank]]
 * (a DeNo chain's channel-major plane: destination p's rows are contiguous), elem_bytes 8 (CF32) or 4.  d_recv receives, for
 * p = 0 .. world-1 in time order, rank p's stripe of MY channel block: [chan_per_rank][stripe_frames[p]] at element offset
 * chan_per_rank * sum_{q<p} stripe_frames[q].  One grouped ncclSend / ncclRecv per peer (every xGMI link carries one block each way). */
int csdr_hybrid_exchange(csdr_comm *c, const void *d_plane, void *d_recv, uint32_t chan_per_rank, const uint32_t *stripe_frames,
                         uint32_t elem_bytes, void *stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* CSDR_H */

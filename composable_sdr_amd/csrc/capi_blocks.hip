// C ABI of libcsdr_hip.so (see include/csdr.h): the handles of the single DSP blocks.  Product code: no CPU fallback,
// nothing from oracle/.  Every handle owns its device memory through `mem` and lives the one life-cycle of capi_internal.h:
// create (or open) = argument checks, NewBlock::open, fill, publish; reset (or rewind) = block_reset; a host call =
// block_host_call around the device entry point; destroy = block_destroy.  State carried in two buffers is a PingPong.
#include "capi_internal.h"

#include <cstdio>
#include <cstring>

using namespace csdr;

// ---------------------------------------------------------------------------
// handles
// ---------------------------------------------------------------------------
struct csdr_dcblock {
    int device; DeviceBuffers mem; uint32_t max_n; DcParams dc;
    float2 *d_state = nullptr, *d_scratch = nullptr, *d_x = nullptr, *d_y = nullptr;
};
struct csdr_nco {
    int device; DeviceBuffers mem; uint32_t max_n; uint32_t theta, d_theta;
    float2 *d_x = nullptr, *d_y = nullptr;
};
struct csdr_agc {
    int device; DeviceBuffers mem; uint32_t C, max_n; AgcParams p; AgcState *d_st = nullptr; float2 *d_z = nullptr;
};
struct csdr_iirfilt {
    int device; DeviceBuffers mem; uint32_t C, max_n; BiquadParams p; PingPong<float2> st; float *d_x = nullptr;
};
struct csdr_firdecim {
    int device; DeviceBuffers mem; uint32_t C, max_n, M, h_len; float *d_h = nullptr; PingPong<float> hist;
    float *d_x = nullptr, *d_y = nullptr;
};
struct csdr_resamp {
    int device; DeviceBuffers mem; uint32_t max_in; ResampDesign d;
    // stage s (s < K: half-band decimators; s == K: the arbitrary stage): history-prefixed input buffer, its tail kept in place
    std::vector<float2 *> d_buf; std::vector<float *> d_h; std::vector<uint32_t> H; std::vector<uint64_t> n_seen;
    float *d_pfb = nullptr; float2 *d_out = nullptr;
    uint64_t t_next = 0;         // Q32.32 absolute time (arbitrary-stage input samples) of the next output
    bool passthrough = false;    // rate 0: the reference's "no resampler" (Liquid.chs:100-103); owns no device memory
};
struct csdr_ampdem {
    int device; DeviceBuffers mem; uint32_t C, max_n; PingPong<float> q; float2 *d_z = nullptr; float *d_f = nullptr;
};
struct csdr_freqdem {
    int device; DeviceBuffers mem; uint32_t C, max_n; float ref; PingPong<float2> rp; float2 *d_z = nullptr; float *d_f = nullptr;
};

extern "C" {

// ---------------------------------------------------------------------------
// dcBlocker
// ---------------------------------------------------------------------------
int csdr_dcblock_create(float alpha, uint32_t max_samples, csdr_dcblock **out)
{
    if (!out || !(alpha > 0.f && alpha < 1.f)) { set_error("dcblock: bad arguments"); return CSDR_ERR_INVALID; }
    NewBlock<csdr_dcblock> h;
    int r = h.open(); if (r) return r;
    h->max_n = block_max_n(max_samples, 1u << 20); h->dc = make_dc(alpha);
    if ((r = block_zeros(h->mem, &h->d_state, 1)) || (r = h->mem.alloc_n(&h->d_scratch, 2 * (size_t)(h->max_n / DC_BLOCK + 2))) ||
        (r = h->mem.alloc_n(&h->d_x, h->max_n)) || (r = h->mem.alloc_n(&h->d_y, h->max_n))) return r;
    return h.publish(out);
}

int csdr_dcblock_process_device(csdr_dcblock *h, const void *d_x, uint32_t n, void *d_y, void *stream)
{
    if (!h) { set_error("dcblock: null handle"); return CSDR_ERR_INVALID; }
    if (int r = block_check_n("dcblock", n, h->max_n)) return r;
    NcoParams nco{};
    return launch_dc_mix((const float2 *)d_x, (float2 *)d_y, n, true, h->dc, h->d_state, h->d_scratch, false, nco,
                         nullptr, (hipStream_t)stream);
}

int csdr_dcblock_process(csdr_dcblock *h, const float *x, uint32_t n, float *y)
{
    if (int r = block_check_call("dcblock", h, x, n, y)) return r;
    if (!n) return CSDR_OK;
    return block_round_trip("dcblock", h->device, h->d_x, x, sizeof(float2) * n, h->d_y, y, sizeof(float2) * n,
                            [&] { return csdr_dcblock_process_device(h, h->d_x, n, h->d_y, nullptr); });
}

int csdr_dcblock_destroy(csdr_dcblock *h) { return block_destroy(h); }

// ---------------------------------------------------------------------------
// mixDown / mixUp
// ---------------------------------------------------------------------------
int csdr_nco_create(float freq, uint32_t max_samples, csdr_nco **out)
{
    if (!out || !std::isfinite(freq)) { set_error("nco: bad arguments"); return CSDR_ERR_INVALID; }
    NewBlock<csdr_nco> h;
    int r = h.open(); if (r) return r;
    h->max_n = block_max_n(max_samples, 1u << 20);
    h->theta = 0; h->d_theta = nco_freq_word(freq);
    if ((r = h->mem.alloc_n(&h->d_x, h->max_n)) || (r = h->mem.alloc_n(&h->d_y, h->max_n))) return r;
    return h.publish(out);
}

static int nco_mix(csdr_nco *h, const float *x, uint32_t n, float *y, int up)
{
    if (int r = block_check_call("nco", h, x, n, y)) return r;
    if (!n) return CSDR_OK;
    const int r = block_round_trip("nco", h->device, h->d_x, x, sizeof(float2) * n, h->d_y, y, sizeof(float2) * n, [&] {
        NcoParams nco{}; nco.theta0 = h->theta; nco.d_theta = h->d_theta; nco.up = up;
        DcParams dc{};
        return launch_dc_mix(h->d_x, h->d_y, n, false, dc, nullptr, nullptr, true, nco, nullptr, nullptr);
    });
    if (!r) h->theta += n * h->d_theta;
    return r;
}
int csdr_nco_mix_down(csdr_nco *h, const float *x, uint32_t n, float *y) { return nco_mix(h, x, n, y, 0); }
int csdr_nco_mix_up(csdr_nco *h, const float *x, uint32_t n, float *y) { return nco_mix(h, x, n, y, 1); }
int csdr_nco_get_words(const csdr_nco *h, uint32_t *theta, uint32_t *d_theta)
{
    if (!h) return CSDR_ERR_INVALID;
    if (theta) *theta = h->theta;
    if (d_theta) *d_theta = h->d_theta;
    return CSDR_OK;
}
int csdr_nco_destroy(csdr_nco *h) { return block_destroy(h); }

// ---------------------------------------------------------------------------
// automaticGainControl (nchan instances)
// ---------------------------------------------------------------------------
int csdr_agc_create(float threshold_db, uint32_t nchan, uint32_t max_samples, csdr_agc **out)
{
    if (!out || !nchan || !std::isfinite(threshold_db)) { set_error("agc: bad arguments"); return CSDR_ERR_INVALID; }
    NewBlock<csdr_agc> h;
    int r = h.open(); if (r) return r;
    h->C = nchan; h->max_n = block_max_n(max_samples); h->p = make_agc(threshold_db);
    if ((r = h->mem.alloc_n(&h->d_st, nchan)) || (r = h->mem.alloc_n(&h->d_z, (size_t)nchan * h->max_n))) return r;
    if ((r = launch_agc_init(h->d_st, nchan, nullptr))) return r;
    CSDR_HIP(hipDeviceSynchronize());
    return h.publish(out);
}
int csdr_agc_process(csdr_agc *h, const float *x, uint32_t n, float *y)
{
    if (int r = block_check_call("agc", h, x, n, y)) return r;
    if (!n) return CSDR_OK;
    const size_t bytes = sizeof(float2) * (size_t)h->C * n;
    return block_round_trip("agc", h->device, h->d_z, x, bytes, h->d_z, y, bytes,
                            [&] { return launch_agc(h->d_z, h->C, n, h->d_st, h->p, nullptr); });
}
int csdr_agc_destroy(csdr_agc *h) { return block_destroy(h); }

// ---------------------------------------------------------------------------
// fmDemodulator (nchan instances)
// ---------------------------------------------------------------------------
int csdr_freqdem_create(float kf, uint32_t nchan, uint32_t max_samples, csdr_freqdem **out)
{
    if (!out || !nchan || !(kf > 0.f)) { set_error("freqdem: bad arguments (kf must be > 0)"); return CSDR_ERR_INVALID; }
    NewBlock<csdr_freqdem> h;
    int r = h.open(); if (r) return r;
    h->C = nchan; h->max_n = block_max_n(max_samples); h->ref = fm_ref_of(kf);
    if ((r = h->rp.alloc_zeroed(h->mem, nchan)) || (r = h->mem.alloc_n(&h->d_z, (size_t)nchan * h->max_n)) ||
        (r = h->mem.alloc_n(&h->d_f, (size_t)nchan * h->max_n))) return r;
    return h.publish(out);
}
int csdr_freqdem_process(csdr_freqdem *h, const float *x, uint32_t n, float *m)
{
    if (int r = block_check_call("freqdem", h, x, n, m)) return r;
    if (!n) return CSDR_OK;
    const size_t Cn = (size_t)h->C * n;
    return block_round_trip("freqdem", h->device, h->d_z, x, sizeof(float2) * Cn, h->d_f, m, sizeof(float) * Cn, [&] {
        return h->rp.flip_behind(launch_fm(h->d_z, h->d_f, h->C, n, h->ref, h->rp.in(), h->rp.out(), nullptr));
    });
}
int csdr_freqdem_destroy(csdr_freqdem *h) { return block_destroy(h); }

// ---------------------------------------------------------------------------
// iirFilter n fc f0 ap as (Liquid.chs:629-638), firDecimator m (Liquid.chs:485-501)
// ---------------------------------------------------------------------------
int csdr_iirfilt_create(uint32_t order, float fc, float f0, float ap, float as_db, uint32_t nchan, uint32_t max_samples, csdr_iirfilt **out)
{
    (void)f0; (void)ap; (void)as_db;
    if (!out || !nchan || !(fc > 0.f && fc < 0.5f)) { set_error("iirfilt: bad arguments (fc in (0, 0.5))"); return CSDR_ERR_INVALID; }
    if (order != 2) { set_error("iirfilt: only the reference's order-2 Butterworth low-pass is built (order %u)", order); return CSDR_ERR_INVALID; }
    NewBlock<csdr_iirfilt> h;
    int r = h.open(); if (r) return r;
    h->C = nchan; h->max_n = block_max_n(max_samples); h->p = design_butter2_lowpass(fc);
    if ((r = h->mem.alloc_n(&h->d_x, (size_t)nchan * h->max_n)) || (r = h->st.alloc_zeroed(h->mem, nchan))) return r;
    return h.publish(out);
}
int csdr_iirfilt_process(csdr_iirfilt *h, const float *x, uint32_t n, float *y)
{
    if (int r = block_check_call("iirfilt", h, x, n, y)) return r;
    if (!n) return CSDR_OK;
    const size_t bytes = sizeof(float) * (size_t)h->C * n;
    return block_round_trip("iirfilt", h->device, h->d_x, x, bytes, h->d_x, y, bytes, [&] {
        return h->st.flip_behind(launch_biquad(h->d_x, h->d_x, h->C, n, h->p, h->st.in(), h->st.out(), nullptr));
    });
}
int csdr_iirfilt_destroy(csdr_iirfilt *h) { return block_destroy(h); }

int csdr_firdecim_create(uint32_t decim, uint32_t nchan, uint32_t max_samples, csdr_firdecim **out)
{
    if (!out || !nchan || decim < 1 || decim > 4096) { set_error("firdecim: bad arguments"); return CSDR_ERR_INVALID; }
    NewBlock<csdr_firdecim> h;
    int r = h.open(); if (r) return r;
    const std::vector<float> taps = design_firdecim_kaiser(decim, 10, 60.0f);          // firdecimCreate, Liquid.chs:485-490
    h->C = nchan; h->max_n = block_max_n(max_samples); h->M = decim; h->h_len = (uint32_t)taps.size();
    const size_t hist = (size_t)nchan * (h->h_len - 1);
    if ((r = h->mem.alloc_n(&h->d_x, (size_t)nchan * h->max_n)) || (r = h->mem.alloc_n(&h->d_y, (size_t)nchan * (h->max_n / decim + 1))) ||
        (r = block_upload(h->mem, &h->d_h, taps.data(), taps.size())) || (r = h->hist.alloc_zeroed(h->mem, hist))) return r;
    return h.publish(out);
}
int csdr_firdecim_process(csdr_firdecim *h, const float *x, uint32_t n, float *y)
{
    if (int r = block_check_call("firdecim", h, x, n, y)) return r;
    if (n % h->M) { set_error("firdecim: %u samples are not a multiple of the decimation %u (Liquid.chs:495-497)", n, h->M); return CSDR_ERR_SIZE; }
    if (!n) return CSDR_OK;
    const size_t C = h->C;
    return block_round_trip("firdecim", h->device, h->d_x, x, sizeof(float) * C * n, h->d_y, y, sizeof(float) * C * (n / h->M), [&] {
        return h->hist.flip_behind(launch_firdecim(h->d_x, h->d_y, h->C, n, h->M, h->d_h, h->h_len, h->hist.in(), h->hist.out(), nullptr));
    });
}
int csdr_firdecim_destroy(csdr_firdecim *h) { return block_destroy(h); }

// ---------------------------------------------------------------------------
// resampler r as (Liquid.chs:56-117)
// ---------------------------------------------------------------------------
int csdr_resamp_create(float rate, float As, uint32_t max_in, csdr_resamp **out)
{
    if (!out || rate < 0.f || !(rate == rate)) { set_error("resamp: bad arguments"); return CSDR_ERR_INVALID; }
    if (rate > 2.0f) { set_error("resamp: rate %g > 2 (interpolating half-band stages are not built)", rate); return CSDR_ERR_INVALID; }
    NewBlock<csdr_resamp> h;
    int r = h.open(); if (r) return r;
    h->max_in = block_max_n(max_in);
    if (rate == 0.f) { h->passthrough = true; return h.publish(out); }
    h->d = design_msresamp(rate, As);
    const uint32_t K = h->d.K, P = 2 * h->d.m_arb;
    h->d_buf.assign(K + 1, nullptr); h->d_h.assign(K, nullptr); h->H.assign(K + 1, 0); h->n_seen.assign(K + 1, 0);
    uint32_t cap = h->max_in;
    for (uint32_t s = 0; s <= K; s++) {
        h->H[s] = s < K ? 4 * h->d.m_hb[s] + 1 : P + 1;
        if ((r = block_zeros(h->mem, &h->d_buf[s], (size_t)h->H[s] + cap + 2))) return r;
        if (s < K) {
            if ((r = block_upload(h->mem, &h->d_h[s], h->d.h_hb[s].data(), h->d.h_hb[s].size()))) return r;
            cap = cap / 2 + 1;
        }
    }
    if ((r = block_upload(h->mem, &h->d_pfb, h->d.pfb.data(), h->d.pfb.size()))) return r;
    if ((r = h->mem.alloc_n(&h->d_out, (size_t)csdr_resamp_max_out(h.get(), h->max_in)))) return r;
    if (!getenv("CSDR_QUIET")) {
        // what msresamp_crcf_print shows in the reference ("Using resampler:", Liquid.chs:105-106)
        printf("csdr resampler: rate=%g = 2^-%u x %g, half-band taps:", rate, K, h->d.rho);
        for (uint32_t s = 0; s < K; s++) printf(" %u", 4 * h->d.m_hb[s] + 1);
        printf(", arbitrary stage: npfb=%u m=%u fc=%g As=%g\n", h->d.npfb, h->d.m_arb, h->d.fc, As);
        fflush(stdout);
    }
    return h.publish(out);
}
float csdr_resamp_get_rate(const csdr_resamp *h) { return h ? (h->passthrough ? 1.0f : h->d.rate) : 0.f; }
uint32_t csdr_resamp_max_out(const csdr_resamp *h, uint32_t n_in)
{
    if (!h) return 0;
    if (h->passthrough) return n_in;
    return 2u * (uint32_t)std::ceil((double)h->d.rate * n_in) + 2u;      // the reference's 2*ceil(r*nx) (Liquid.chs:81)
}
// the checks both entry points start with; *n_out = 0, and nothing more to do for an empty call
static int resamp_check(const csdr_resamp *h, const void *x, uint32_t n_in, const void *y, uint32_t *n_out)
{
    if (!h || !n_out) return block_null_arg("resamp");
    *n_out = 0;
    if (!n_in) return CSDR_OK;
    if (!x || !y) { set_error("resamp: null buffer"); return CSDR_ERR_INVALID; }
    return block_check_n("resamp", n_in, h->max_in);
}
int csdr_resamp_process_device(csdr_resamp *h, const void *d_x, uint32_t n_in, void *d_y, uint32_t *n_out, void *stream)
{
    int r = resamp_check(h, d_x, n_in, d_y, n_out);
    if (r || !n_in) return r;
    DevGuard guard(h->device);
    hipStream_t s = (hipStream_t)stream;
    if (h->passthrough) {
        CSDR_HIP(hipMemcpyAsync(d_y, d_x, sizeof(float2) * (size_t)n_in, hipMemcpyDeviceToDevice, s));
        *n_out = n_in;
        return CSDR_OK;
    }
    const uint32_t K = h->d.K, P = 2 * h->d.m_arb;
    if ((const void *)(h->d_buf[0] + h->H[0]) != d_x)
        CSDR_HIP(hipMemcpyAsync(h->d_buf[0] + h->H[0], d_x, sizeof(float2) * (size_t)n_in, hipMemcpyDeviceToDevice, s));
    uint32_t n = n_in;
    for (uint32_t st = 0; st < K; st++) {
        // stage input: absolute samples [N0 - H, N0 + n) sit at buffer positions [0, H + n); output j = sum h[i] x[2j+1-i]
        const uint64_t N0 = h->n_seen[st], N1 = N0 + n;
        const uint32_t ny = (uint32_t)(N1 / 2 - N0 / 2);
        const uint32_t base0 = (uint32_t)((2 * (N0 / 2) + 1) - N0 + h->H[st]);
        float2 *dst = h->d_buf[st + 1] + h->H[st + 1];
        if ((r = launch_hb_decim(h->d_buf[st], h->d_h[st], dst, ny, base0, h->d.m_hb[st], s))) return r;
        if ((r = launch_keep_tail(h->d_buf[st], h->H[st], n, s))) return r;
        h->n_seen[st] = N1;
        n = ny;
    }
    {
        const uint64_t N0 = h->n_seen[K], N1 = N0 + n;
        uint32_t ny = 0;
        if (N1 >= 2) {
            // outputs while floor(t) + 1 <= N1 - 1, i.e. t < (N1 - 1) * 2^32
            const uint64_t lim = (N1 - 1) << 32;
            if (h->t_next < lim) ny = (uint32_t)((lim - h->t_next + h->d.delta - 1) / h->d.delta);
        }
        // buffer position of absolute sample a is a - (N0 - H)
        const uint64_t t_first = h->t_next - (N0 << 32) + ((uint64_t)h->H[K] << 32);
        if ((r = launch_resamp_arb(h->d_buf[K], h->d_pfb, (float2 *)d_y, ny, t_first, h->d.delta, h->d.npfb, P, s))) return r;
        if ((r = launch_keep_tail(h->d_buf[K], h->H[K], n, s))) return r;
        h->t_next += (uint64_t)ny * h->d.delta;
        h->n_seen[K] = N1;
        *n_out = ny;
    }
    return CSDR_OK;
}
int csdr_resamp_process(csdr_resamp *h, const float *x, uint32_t n_in, float *y, uint32_t *n_out)
{
    int r = resamp_check(h, x, n_in, y, n_out);
    if (r || !n_in) return r;
    if (h->passthrough) { memcpy(y, x, sizeof(float2) * (size_t)n_in); *n_out = n_in; return CSDR_OK; }
    DevGuard guard;
    if ((r = block_select("resamp", guard, h->device))) return r;
    // the first stage's buffer doubles as the H2D landing area
    float2 *stage0 = h->d_buf[0] + h->H[0];
    CSDR_HIP(hipMemcpy(stage0, x, sizeof(float2) * (size_t)n_in, hipMemcpyHostToDevice));
    // process_device copies d_x into the same place: skip that by handing it the landing area itself
    uint32_t no = 0;
    if ((r = csdr_resamp_process_device(h, stage0, n_in, h->d_out, &no, nullptr))) return r;
    CSDR_HIP(hipMemcpy(y, h->d_out, sizeof(float2) * (size_t)no, hipMemcpyDeviceToHost));
    *n_out = no;
    return CSDR_OK;
}
int csdr_resamp_destroy(csdr_resamp *h) { return block_destroy(h); }

// ---------------------------------------------------------------------------
// amDemodulator (Liquid.chs:439-469)
// ---------------------------------------------------------------------------
int csdr_ampdem_create(float mod_index, uint32_t nchan, uint32_t max_samples, csdr_ampdem **out)
{
    if (!out || !nchan || !(mod_index > 0.f)) { set_error("ampdem: bad arguments (mod_index must be > 0)"); return CSDR_ERR_INVALID; }
    NewBlock<csdr_ampdem> h;
    int r = h.open(); if (r) return r;
    h->C = nchan; h->max_n = block_max_n(max_samples);
    if ((r = h->mem.alloc_n(&h->d_z, (size_t)nchan * h->max_n)) || (r = h->mem.alloc_n(&h->d_f, (size_t)nchan * h->max_n)) ||
        (r = h->q.alloc_zeroed(h->mem, nchan))) return r;
    return h.publish(out);
}
int csdr_ampdem_process(csdr_ampdem *h, const float *x, uint32_t n, float *m)
{
    if (int r = block_check_call("ampdem", h, x, n, m)) return r;
    if (!n) return CSDR_OK;
    const size_t Cn = (size_t)h->C * n;
    return block_round_trip("ampdem", h->device, h->d_z, x, sizeof(float2) * Cn, h->d_f, m, sizeof(float) * Cn, [&] {
        return h->q.flip_behind(launch_am(h->d_z, h->d_f, h->C, n, h->q.in(), h->q.out(), 0.01f, nullptr));
    });
}
int csdr_ampdem_destroy(csdr_ampdem *h) { return block_destroy(h); }

// ---------------------------------------------------------------------------
// stereoFMDecoder quadRate decim (Liquid.chs:959-1078), nchan independent streams
// ---------------------------------------------------------------------------
}  // extern "C"
struct csdr_fmstereo {
    // cur: the one index of the three pairs d_xh, d_ub, d_dh (no PingPong: FmsBufs / FmsLaunch take both sides and the index)
    int device; DeviceBuffers mem; uint32_t C, max_n, M; FmsDesign f; uint32_t theta = 0; int cur = 0;
    float *d_hp = nullptr, *d_ha = nullptr, *d_hdec = nullptr, *d_xh[2] = {nullptr, nullptr}, *d_ub[2] = {nullptr, nullptr};
    float2 *d_p = nullptr, *d_bq = nullptr; float *d_lpr = nullptr, *d_lr = nullptr, *d_dh[2] = {nullptr, nullptr}; uint2 *d_pll = nullptr;
    float *d_in = nullptr, *d_out = nullptr;
    hipEvent_t ev[6] = {}; bool timed = false;
    ~csdr_fmstereo() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    uint32_t Hx() const { return f.N - 1 + f.d; }
    uint32_t ustride() const { return f.N - 1 + max_n; }
};
static int fms_init_state(csdr_fmstereo *h)
{
    const uint32_t C = h->C, Hd = (uint32_t)h->f.h_dec.size() - 1;
    for (int i = 0; i < 2; i++) {
        CSDR_HIP(hipMemset(h->d_xh[i], 0, sizeof(float) * (size_t)C * h->Hx()));
        CSDR_HIP(hipMemset(h->d_ub[i], 0, sizeof(float) * (size_t)C * h->ustride()));
        CSDR_HIP(hipMemset(h->d_dh[i], 0, sizeof(float) * (size_t)2 * C * Hd));
    }
    CSDR_HIP(hipMemset(h->d_bq, 0, sizeof(float2) * 2 * (size_t)C));
    std::vector<uint2> pll(C, make_uint2(0u, h->f.d_nco));           // ncoPE: theta 0, d_theta = constrain(ncoF)
    CSDR_HIP(hipMemcpy(h->d_pll, pll.data(), sizeof(uint2) * C, hipMemcpyHostToDevice));
    h->theta = 0; h->cur = 0;
    return 0;
}
extern "C" {
int csdr_fmstereo_destroy(csdr_fmstereo *h) { return block_destroy(h); }
int csdr_fmstereo_create(float quad_rate, uint32_t decim, uint32_t nchan, uint32_t max_samples, csdr_fmstereo **out)
{
    if (!out || !nchan || decim < 1 || decim > 4096 || !(quad_rate >= 40000.f && quad_rate <= 2.7e6f)) {
        set_error("fmstereo: bad arguments (quad_rate in [40e3, 2.7e6]: the 19 kHz pilot below Nyquist, FIRs of <= 2000 taps; decim in [1, 4096])");
        return CSDR_ERR_INVALID;
    }
    NewBlock<csdr_fmstereo> h;
    int r = h.open(); if (r) return r;
    h->C = nchan; h->max_n = block_max_n(max_samples); h->M = decim;
    h->f = design_fmstereo((double)quad_rate, decim);
    h->timed = diag_env("CSDR_FMS_TIME") != nullptr;           // hipEvents around the five kernels (tools/fms_time.py)
    const size_t C = nchan, N = h->f.N, Hd = h->f.h_dec.size() - 1, n = h->max_n;
    DeviceBuffers &mem = h->mem;
    if ((r = block_upload(mem, &h->d_hp, h->f.h_pilot.data(), N)) || (r = block_upload(mem, &h->d_ha, h->f.h_audio.data(), N)) ||
        (r = block_upload(mem, &h->d_hdec, h->f.h_dec.data(), h->f.h_dec.size())) ||
        (r = mem.alloc_n(&h->d_xh[0], C * h->Hx())) || (r = mem.alloc_n(&h->d_xh[1], C * h->Hx())) ||
        (r = mem.alloc_n(&h->d_ub[0], C * h->ustride())) || (r = mem.alloc_n(&h->d_ub[1], C * h->ustride())) ||
        (r = mem.alloc_n(&h->d_p, C * n)) || (r = mem.alloc_n(&h->d_lpr, C * n)) || (r = mem.alloc_n(&h->d_lr, 2 * C * n)) ||
        (r = mem.alloc_n(&h->d_bq, 2 * C)) || (r = mem.alloc_n(&h->d_dh[0], 2 * C * Hd)) || (r = mem.alloc_n(&h->d_dh[1], 2 * C * Hd)) ||
        (r = mem.alloc_n(&h->d_pll, C)) || (r = mem.alloc_n(&h->d_in, C * n)) || (r = mem.alloc_n(&h->d_out, 2 * C * (n / decim))))
        return r;
    if ((r = fms_init_state(h.get()))) return r;
    return h.publish(out);
}
int csdr_fmstereo_process_device(csdr_fmstereo *h, const void *d_mpx, uint32_t n, void *d_lr, uint32_t *n_out, void *stream)
{
    if (!h || !n_out) return block_null_arg("fmstereo");
    if (int r = block_check_n("fmstereo", n, h->max_n)) return r;
    *n_out = h->C * 2 * (n / h->M);
    if (!n) return CSDR_OK;
    if (!d_mpx || !d_lr) { set_error("fmstereo: null buffer"); return CSDR_ERR_INVALID; }
    FmsBufs b{h->d_hp, h->d_ha, h->d_hdec, {h->d_xh[0], h->d_xh[1]}, {h->d_ub[0], h->d_ub[1]}, h->d_p, h->d_lpr, h->d_lr, h->d_pll, h->d_bq,
              {h->d_dh[0], h->d_dh[1]}};
    FmsLaunch l{h->C, n, h->f.N, h->f.d, h->M, (uint32_t)h->f.h_dec.size(), h->ustride(), h->theta, h->f.d_nco, h->cur,
                h->f.scale_pilot, h->f.scale_audio, h->f.alpha, h->f.beta, h->f.bq.b0, h->f.bq.b1, h->f.bq.b2, h->f.bq.a1, h->f.bq.a2};
    const bool timed = h->timed;
    if (timed && !h->ev[0])
        for (hipEvent_t &e : h->ev) CSDR_HIP(hipEventCreate(&e));
    int r = launch_fmstereo((const float *)d_mpx, (float *)d_lr, b, l, (hipStream_t)stream, timed ? h->ev : nullptr);
    if (r) return r;
    h->theta += n * h->f.d_nco;
    h->cur ^= 1;
    return CSDR_OK;
}
int csdr_fmstereo_process(csdr_fmstereo *h, const float *mpx, uint32_t n, float *lr, uint32_t *n_out)
{
    if (!n_out) return block_null_arg("fmstereo");
    if (int r = block_check_call("fmstereo", h, mpx, n, lr)) return r;
    *n_out = h->C * 2 * (n / h->M);
    if (!n) return CSDR_OK;
    return block_round_trip("fmstereo", h->device, h->d_in, mpx, sizeof(float) * (size_t)h->C * n, h->d_out, lr, sizeof(float) * (size_t)*n_out,
                            [&] { return csdr_fmstereo_process_device(h, h->d_in, n, h->d_out, n_out, nullptr); });
}
int csdr_fmstereo_reset(csdr_fmstereo *h) { return block_reset(h, [&] { return fms_init_state(h); }); }
uint32_t csdr_fmstereo_get_delay(const csdr_fmstereo *h) { return h ? h->f.d : 0; }
uint32_t csdr_fmstereo_get_taps_len(const csdr_fmstereo *h) { return h ? h->f.N : 0; }
int csdr_fmstereo_get_pll(csdr_fmstereo *h, uint32_t chan, uint32_t *theta, uint32_t *d_theta)
{
    if (!h || chan >= h->C) { set_error("fmstereo: bad channel"); return CSDR_ERR_INVALID; }
    DevGuard guard(h->device);
    uint2 w;
    CSDR_HIP(hipMemcpy(&w, h->d_pll + chan, sizeof(uint2), hipMemcpyDeviceToHost));
    if (theta) *theta = w.x;
    if (d_theta) *d_theta = w.y;
    return CSDR_OK;
}
int csdr_fmstereo_kernel_times(csdr_fmstereo *h, float *us5)
{
    if (!h || !us5) return CSDR_ERR_INVALID;
    if (!h->ev[0]) { set_error("fmstereo: kernel timing needs CSDR_DIAG=1 CSDR_FMS_TIME=1 at create"); return CSDR_ERR_INVALID; }
    DevGuard guard(h->device);
    CSDR_HIP(hipEventSynchronize(h->ev[5]));
    for (int i = 0; i < 5; i++) { float ms = 0.f; CSDR_HIP(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1])); us5[i] = 1000.f * ms; }
    return CSDR_OK;
}

// ---------------------------------------------------------------------------
// symSyncR k m beta M (Liquid.chs:244-282): symsync_rrrf on nchan independent streams
// ---------------------------------------------------------------------------
}  // extern "C"
struct csdr_symsync {
    int device; DeviceBuffers mem; uint32_t C, max_n; SymsyncDesign d;
    float *d_mf = nullptr, *d_dmf = nullptr, *d_hist = nullptr, *d_x = nullptr, *d_y = nullptr;
    SymsyncState *d_st = nullptr; uint32_t *d_ny = nullptr, *d_fault = nullptr;    // state and windows are updated in place: no pair
    // the sample type, fixed by the first process call after create, reset or a setter: 0 open, 1 F32 rows, 2 CF32 rows
    int kind = 0;
    float2 *d_histc = nullptr, *d_xc = nullptr, *d_yc = nullptr;    // the complex windows and staging: allocated by the first complex call
};
static int symsync_init_state(csdr_symsync *h)
{
    CSDR_HIP(hipMemset(h->d_hist, 0, sizeof(float) * (size_t)h->C * (h->d.L - 1)));
    if (h->d_histc) CSDR_HIP(hipMemset(h->d_histc, 0, sizeof(float2) * (size_t)h->C * (h->d.L - 1)));
    h->kind = 0;
    std::vector<SymsyncState> st(h->C, h->d.init);
    CSDR_HIP(hipMemcpy(h->d_st, st.data(), sizeof(SymsyncState) * h->C, hipMemcpyHostToDevice));
    CSDR_HIP(hipMemset(h->d_fault, 0, sizeof(uint32_t)));
    return 0;
}
// the handle's sample type: the first process call fixes it, the other kind of call is refused with nothing touched
static int symsync_take_kind(csdr_symsync *h, int kind)
{
    if (h->kind && h->kind != kind) {
        set_error("symsync: the handle processes %s rows since its first call; reset, set_taps or set_rnyquist reopens the choice",
                  h->kind == 1 ? "F32" : "CF32");
        return CSDR_ERR_INVALID;
    }
    h->kind = kind;
    return CSDR_OK;
}
// the checks in front of a complex call, and the complex windows the first one allocates (on the handle's device)
static int symsync_complex_ready(csdr_symsync *h, uint32_t n, bool host)
{
    if (int r = block_check_n("symsync", n, h->max_n)) return r;
    const size_t lds = symsyncc_lds_bytes(h->d.L, h->d.M);
    if (lds > SYMSYNCC_MAX_LDS) {
        set_error("symsync: complex rows need 8 (2 k m) npfb + 512 ((2 k m + 31) | 1) = %zu bytes of LDS, the limit is %zu", lds,
                  SYMSYNCC_MAX_LDS);
        return CSDR_ERR_INVALID;
    }
    int r = symsync_take_kind(h, 2); if (r) return r;
    if (h->d_histc && (!host || h->d_xc)) return CSDR_OK;
    DevGuard guard;
    if ((r = block_select("symsync", guard, h->device))) return r;
    const size_t C = h->C;
    if (!h->d_histc && (r = block_zeros(h->mem, &h->d_histc, C * (h->d.L - 1)))) return r;
    if (host && !h->d_xc && ((r = h->mem.alloc_n(&h->d_xc, C * h->max_n)) || (r = h->mem.alloc_n(&h->d_yc, C * h->max_n)))) return r;
    return CSDR_OK;
}
static int symsync_launch_c(csdr_symsync *h, const void *d_x, uint32_t n, void *d_y, void *d_ny, void *stream)
{
    const SymsyncDesign &d = h->d;
    SymsyncLaunch l{h->C, n, n, d.L, d.M, d.k_out, (float)d.k, d.b0, d.b1, d.b2, d.a1, d.a2, d.rate_adj};
    return launch_symsyncc((const float2 *)d_x, (float2 *)d_y, (uint32_t *)d_ny, h->d_mf, h->d_dmf, h->d_histc, h->d_st, h->d_fault, l,
                           (hipStream_t)stream);
}
// the host side of both calls: rows of row_bytes in (none for n = 0), run(), then the counts, the fault word and the rows out
template <class Run>
static int symsync_host_call(csdr_symsync *h, void *d_x, const float *x, size_t row_bytes, const void *d_y, float *y, uint32_t *ny, Run run)
{
    uint32_t fault = 0;
    const int r = block_host_call("symsync", h->device, d_x, x, row_bytes, run,
                                  {{ny, h->d_ny, sizeof(uint32_t) * h->C}, {&fault, h->d_fault, sizeof(uint32_t)}, {y, d_y, row_bytes}});
    if (r) return r;
    if (fault) { set_error("symsync: a stream is faulted (del <= 0 or more than n outputs in a call); reset clears it"); return CSDR_ERR_SIZE; }
    return CSDR_OK;
}
extern "C" {
int csdr_symsync_destroy(csdr_symsync *h) { return block_destroy(h); }
int csdr_symsync_create(uint32_t k, uint32_t m, float beta, uint32_t npfb, float lf_bw, uint32_t k_out, uint32_t nchan,
                        uint32_t max_samples, csdr_symsync **out)
{
    const uint64_t L = 2ull * k * m;
    if (!out || !nchan || k_out < 1 || k < k_out || m < 1 || L > SYMSYNC_MAX_SUB || npfb < 1 || npfb > SYMSYNC_MAX_PFB ||
        L * npfb > SYMSYNC_MAX_BANK || !(lf_bw >= 0.f && lf_bw <= 1.f)) {
        set_error("symsync: bad arguments (k >= k_out >= 1, m >= 1, 2 k m <= %u, npfb in [1, %u], 2 k m npfb <= %u, lf_bw in [0, 1])",
                  SYMSYNC_MAX_SUB, SYMSYNC_MAX_PFB, SYMSYNC_MAX_BANK);
        return CSDR_ERR_INVALID;
    }
    NewBlock<csdr_symsync> h;
    int r = h.open(); if (r) return r;
    h->C = nchan; h->max_n = block_max_n(max_samples);
    h->d = design_symsync_kaiser(k, m, beta, npfb, lf_bw, k_out);
    const size_t C = nchan, n = h->max_n, LM = h->d.mf.size();
    DeviceBuffers &mem = h->mem;
    if ((r = block_upload(mem, &h->d_mf, h->d.mf.data(), LM)) || (r = block_upload(mem, &h->d_dmf, h->d.dmf.data(), LM)) ||
        (r = mem.alloc_n(&h->d_hist, C * (h->d.L - 1))) || (r = mem.alloc_n(&h->d_st, C)) || (r = mem.alloc_n(&h->d_ny, C)) ||
        (r = mem.alloc_n(&h->d_fault, 1)) || (r = mem.alloc_n(&h->d_x, C * n)) || (r = mem.alloc_n(&h->d_y, C * n)))
        return r;
    if ((r = symsync_init_state(h.get()))) return r;
    return h.publish(out);
}
int csdr_symsync_process_device(csdr_symsync *h, const void *d_x, uint32_t n, void *d_y, void *d_ny, void *stream)
{
    if (!h || !d_ny) return block_null_arg("symsync");
    if (int r = block_check_n("symsync", n, h->max_n)) return r;
    if (n && (!d_x || !d_y)) { set_error("symsync: null buffer"); return CSDR_ERR_INVALID; }
    if (int r = symsync_take_kind(h, 1)) return r;
    const SymsyncDesign &d = h->d;
    SymsyncLaunch l{h->C, n, n, d.L, d.M, d.k_out, (float)d.k, d.b0, d.b1, d.b2, d.a1, d.a2, d.rate_adj};
    return launch_symsync((const float *)d_x, (float *)d_y, (uint32_t *)d_ny, h->d_mf, h->d_dmf, h->d_hist, h->d_st, h->d_fault, l,
                          (hipStream_t)stream);
}
int csdr_symsync_process(csdr_symsync *h, const float *x, uint32_t n, float *y, uint32_t *ny)
{
    if (!ny) return block_null_arg("symsync");
    if (int r = block_check_call("symsync", h, x, n, y)) return r;
    return symsync_host_call(h, h->d_x, x, sizeof(float) * (size_t)h->C * n, h->d_y, y, ny,
                             [&] { return csdr_symsync_process_device(h, h->d_x, n, h->d_y, h->d_ny, nullptr); });
}
int csdr_symsync_process_c_device(csdr_symsync *h, const void *d_x, uint32_t n, void *d_y, void *d_ny, void *stream)
{
    if (!h || !d_ny) return block_null_arg("symsync");
    if (n && (!d_x || !d_y)) { set_error("symsync: null buffer"); return CSDR_ERR_INVALID; }
    if (int r = symsync_complex_ready(h, n, false)) return r;
    return symsync_launch_c(h, d_x, n, d_y, d_ny, stream);
}
int csdr_symsync_process_c(csdr_symsync *h, const float *x, uint32_t n, float *y, uint32_t *ny)
{
    if (!ny) return block_null_arg("symsync");
    int r = block_check_call("symsync", h, x, n, y); if (r) return r;
    if ((r = symsync_complex_ready(h, n, true))) return r;
    return symsync_host_call(h, h->d_xc, x, sizeof(float2) * (size_t)h->C * n, h->d_yc, y, ny,
                             [&] { return symsync_launch_c(h, h->d_xc, n, h->d_yc, h->d_ny, nullptr); });
}
// symsync_create(k, M, H, H_len) behind create: new banks from the caller's prototype, then the state right after create
int csdr_symsync_set_taps(csdr_symsync *h, const float *H, uint32_t H_len)
{
    if (!h || !H) return block_null_arg("symsync");
    if (H_len != h->d.H_len) { set_error("symsync: %u prototype taps, the handle takes 2 npfb k m + 1 = %u", H_len, h->d.H_len); return CSDR_ERR_INVALID; }
    bool ok = false;
    for (uint32_t i = 0; i < H_len; i++) {
        if (!std::isfinite(H[i])) { ok = false; break; }
        if (H[i] != 0.f) ok = true;
    }
    if (!ok) { set_error("symsync: the prototype taps must be finite and not all zero"); return CSDR_ERR_INVALID; }
    DevGuard guard;
    if (int r = block_select("symsync", guard, h->device)) return r;
    return block_idle_run([&] {
        h->d.H.assign(H, H + H_len);
        symsync_set_prototype(h->d);
        const size_t LM = h->d.mf.size();
        CSDR_HIP(hipMemcpy(h->d_mf, h->d.mf.data(), sizeof(float) * LM, hipMemcpyHostToDevice));
        CSDR_HIP(hipMemcpy(h->d_dmf, h->d.dmf.data(), sizeof(float) * LM, hipMemcpyHostToDevice));
        return symsync_init_state(h);
    });
}
// symsync_create_rnyquist(ftype, k, m, beta, npfb): the prototype at k npfb samples per symbol
int csdr_symsync_set_rnyquist(csdr_symsync *h, int ftype, float beta)
{
    if (!h) return block_null_arg("symsync");
    std::vector<float> H(h->d.H_len);
    if (int r = csdr_firdes_rnyquist(ftype, h->d.k * h->d.M, h->d.m, beta, 0.f, H.data())) return r;
    return csdr_symsync_set_taps(h, H.data(), h->d.H_len);
}
int csdr_symsync_reset(csdr_symsync *h) { return block_reset(h, [&] { return symsync_init_state(h); }); }
int csdr_symsync_get_state(csdr_symsync *h, uint32_t chan, float *tau, float *rate, float *del, float *q_hat)
{
    if (!h || chan >= h->C) { set_error("symsync: bad channel"); return CSDR_ERR_INVALID; }
    DevGuard guard(h->device);
    SymsyncState s;
    CSDR_HIP(hipMemcpy(&s, h->d_st + chan, sizeof(SymsyncState), hipMemcpyDeviceToHost));
    if (tau) *tau = s.tau;
    if (rate) *rate = s.rate;
    if (del) *del = s.del;
    if (q_hat) *q_hat = s.q_hat;
    if (s.fault) { set_error("symsync: stream %u is faulted", chan); return CSDR_ERR_SIZE; }
    return CSDR_OK;
}
uint32_t csdr_symsync_get_taps_len(const csdr_symsync *h) { return h ? h->d.L : 0; }
int csdr_symsync_get_taps(const csdr_symsync *h, float *mf, float *dmf)
{
    if (!h) return CSDR_ERR_INVALID;
    if (mf) std::memcpy(mf, h->d.mf.data(), sizeof(float) * h->d.mf.size());
    if (dmf) std::memcpy(dmf, h->d.dmf.data(), sizeof(float) * h->d.dmf.size());
    return CSDR_OK;
}

// ---------------------------------------------------------------------------
// realToComplex / complexToReal (Liquid.chs:503-546): firhilbf as a 2:1 decimator and a 1:2 interpolator
// ---------------------------------------------------------------------------
}  // extern "C"
struct csdr_firhilb {
    int device; DeviceBuffers mem; uint32_t m, max_n; std::vector<float> hq;
    PingPong<float> hist;                                   // the windows, pair-interleaved (w1[j], w0[j]): [4 m]
    float *d_x = nullptr, *d_y = nullptr;
};
static int firhilb_run(csdr_firhilb *h, bool interp, const void *d_x, uint32_t n, void *d_y, void *stream)
{
    if (!h) return block_null_arg("firhilb");
    if (int r = block_check_n("firhilb", n, h->max_n)) return r;
    if (!n) return CSDR_OK;
    if (!d_x || !d_y || d_x == d_y) { set_error("firhilb: null or aliased buffer"); return CSDR_ERR_INVALID; }
    FirhilbLaunch l{};
    l.n = n; l.m = h->m;
    std::memcpy(l.hq, h->hq.data(), sizeof(float) * h->hq.size());
    return h->hist.flip_behind(launch_firhilb(interp, (const float *)d_x, (float *)d_y, h->hist.in(), h->hist.out(), l, (hipStream_t)stream));
}
static int firhilb_host(csdr_firhilb *h, bool interp, const float *x, uint32_t n, float *y)
{
    if (int r = block_check_call("firhilb", h, x, n, y)) return r;
    if (!n) return CSDR_OK;
    const size_t bytes = sizeof(float) * 2 * (size_t)n;
    return block_round_trip("firhilb", h->device, h->d_x, x, bytes, h->d_y, y, bytes,
                            [&] { return firhilb_run(h, interp, h->d_x, n, h->d_y, nullptr); });
}
extern "C" {
int csdr_firhilb_destroy(csdr_firhilb *h) { return block_destroy(h); }
int csdr_firhilb_create(uint32_t m, float as_db, uint32_t max_samples, csdr_firhilb **out)
{
    if (!out || m < 2 || m > FIRHILB_MAX_M || !(as_db > 0.f) || max_samples > (1u << 30)) {
        set_error("firhilb: bad arguments (m in [2, %u], As > 0, max_samples <= 2^30)", FIRHILB_MAX_M);
        return CSDR_ERR_INVALID;
    }
    NewBlock<csdr_firhilb> h;
    int r = h.open(); if (r) return r;
    h->m = m; h->max_n = block_max_n(max_samples);
    h->hq = design_firhilb(m, as_db);
    const size_t n2 = 2 * (size_t)h->max_n;
    if ((r = h->hist.alloc_zeroed(h->mem, 4 * m)) || (r = h->mem.alloc_n(&h->d_x, n2)) || (r = h->mem.alloc_n(&h->d_y, n2))) return r;
    return h.publish(out);
}
int csdr_firhilb_decim_device(csdr_firhilb *h, const void *d_x, uint32_t n, void *d_y, void *stream)
{
    return firhilb_run(h, false, d_x, n, d_y, stream);
}
int csdr_firhilb_interp_device(csdr_firhilb *h, const void *d_x, uint32_t n, void *d_y, void *stream)
{
    return firhilb_run(h, true, d_x, n, d_y, stream);
}
int csdr_firhilb_decim(csdr_firhilb *h, const float *x_f32, uint32_t n, float *y_cf32) { return firhilb_host(h, false, x_f32, n, y_cf32); }
int csdr_firhilb_interp(csdr_firhilb *h, const float *x_cf32, uint32_t n, float *y_f32) { return firhilb_host(h, true, x_cf32, n, y_f32); }
int csdr_firhilb_reset(csdr_firhilb *h) { return block_reset(h, [&] { return h->hist.reset(nullptr); }); }
uint32_t csdr_firhilb_get_taps_len(const csdr_firhilb *h) { return h ? 2 * h->m : 0; }
int csdr_firhilb_get_taps(const csdr_firhilb *h, float *hq)
{
    if (!h || !hq) return CSDR_ERR_INVALID;
    std::memcpy(hq, h->hq.data(), sizeof(float) * h->hq.size());
    return CSDR_OK;
}

// ---------------------------------------------------------------------------
// fskDemodulator m k bw (Liquid.chs:336-382): fskdem on nchan independent CF32 streams
// ---------------------------------------------------------------------------
}  // extern "C"
struct csdr_fskdem {
    int device; DeviceBuffers mem; uint32_t C, max_n; FskdemDesign d;
    float2 *d_W = nullptr, *d_x = nullptr; uint32_t *d_map = nullptr, *d_sym = nullptr;
    float *d_e = nullptr;                                   // host-path energies: allocated by the first call that asks for them
};
extern "C" {
int csdr_fskdem_destroy(csdr_fskdem *h) { return block_destroy(h); }
int csdr_fskdem_create(uint32_t m, uint32_t k, float bandwidth, uint32_t nchan, uint32_t max_samples, csdr_fskdem **out)
{
    if (!out || !nchan || m < 1 || m > FSKDEM_MAX_M || k < 2 || k > FSKDEM_MAX_K || !(bandwidth > 0.f && bandwidth < 0.5f)) {
        set_error("fskdem: bad arguments (m in [1, %u], k in [2, %u], bandwidth in (0, 0.5), nchan >= 1)", FSKDEM_MAX_M, FSKDEM_MAX_K);
        return CSDR_ERR_INVALID;
    }
    NewBlock<csdr_fskdem> h;
    int r = h.open(); if (r) return r;
    h->C = nchan; h->max_n = block_max_n(max_samples);
    h->d = design_fskdem(m, k, bandwidth);
    if (h->d.repeated && !getenv("CSDR_QUIET"))
        fprintf(stderr, "csdr_fskdem_create(%u, %u, %g): warning, the demodulation map is not unique (K = %u); consider a larger bandwidth or k\n",
                m, k, (double)bandwidth, h->d.K);
    const size_t C = nchan, n = h->max_n;
    if ((r = block_upload(h->mem, &h->d_W, (const float2 *)h->d.W.data(), h->d.K)) ||
        (r = block_upload(h->mem, &h->d_map, h->d.map.data(), h->d.M)) || (r = h->mem.alloc_n(&h->d_x, C * n)) ||
        (r = h->mem.alloc_n(&h->d_sym, C * (n / k)))) return r;
    return h.publish(out);
}
int csdr_fskdem_process_device(csdr_fskdem *h, const void *d_x, uint32_t n, void *d_sym, void *d_energy, void *stream)
{
    if (!h) return block_null_arg("fskdem");
    if (int r = block_check_n("fskdem", n, h->max_n)) return r;
    if (n / h->d.k == 0) return CSDR_OK;
    if (!d_x || !d_sym) { set_error("fskdem: null buffer"); return CSDR_ERR_INVALID; }
    const FskdemLaunch l{h->C, n, h->d.k, h->d.K, h->d.M};
    return launch_fskdem((const float2 *)d_x, (uint32_t *)d_sym, (float *)d_energy, h->d_W, h->d_map, l, (hipStream_t)stream);
}
int csdr_fskdem_process(csdr_fskdem *h, const float *x, uint32_t n, uint32_t *sym, float *energy, uint32_t *n_out)
{
    if (!h || !n_out) return block_null_arg("fskdem");
    int r = block_check_n("fskdem", n, h->max_n); if (r) return r;
    const size_t ns = n / h->d.k, C = h->C;
    *n_out = (uint32_t)(C * ns);
    if (!ns) return CSDR_OK;
    if (!x || !sym) { set_error("fskdem: null buffer"); return CSDR_ERR_INVALID; }
    if (energy && (r = block_lazy_alloc("fskdem", h->device, h->mem, &h->d_e, C * (h->max_n / h->d.k) * h->d.M))) return r;
    return block_host_call("fskdem", h->device, h->d_x, x, sizeof(float2) * C * n,
                           [&] { return csdr_fskdem_process_device(h, h->d_x, n, h->d_sym, energy ? h->d_e : nullptr, nullptr); },
                           {{sym, h->d_sym, sizeof(uint32_t) * C * ns}, {energy, h->d_e, sizeof(float) * C * ns * h->d.M}});
}
int csdr_fskdem_get_design(const csdr_fskdem *h, uint32_t *K, uint32_t *demod_map)
{
    if (!h) return block_null_arg("fskdem");
    if (K) *K = h->d.K;
    if (demod_map) std::memcpy(demod_map, h->d.map.data(), sizeof(uint32_t) * h->d.M);
    return CSDR_OK;
}

// ---------------------------------------------------------------------------
// firFilterCKaiser / firFilterC / firFilterR (Liquid.chs:868-916, 955-957): firfilt_crcf / firfilt_rrrf on nchan independent
// rows; the two design functions need no GPU
// ---------------------------------------------------------------------------
static bool firdes_kaiser_args_ok(uint32_t n, float fc, float as_db, float mu)
{
    return n >= 2 && n <= FIRFILT_MAX_LEN && fc > 0.f && fc <= 0.5f && as_db > 0.f && mu == 0.f;
}
int csdr_firdes_kaiser(uint32_t n, float fc, float as_db, float mu, float *h)
{
    if (!h || !firdes_kaiser_args_ok(n, fc, as_db, mu)) {
        set_error("firdes_kaiser: bad arguments (n in [2, %u], fc in (0, 0.5], As > 0, mu == 0)", FIRFILT_MAX_LEN);
        return CSDR_ERR_INVALID;
    }
    const std::vector<float> t = design_firfilt_kaiser(n, fc, as_db);
    std::memcpy(h, t.data(), sizeof(float) * n);
    return CSDR_OK;
}
int csdr_firdes_rnyquist(int ftype, uint32_t k, uint32_t m, float beta, float dt, float *h)
{
    const uint64_t n = 2ull * k * m + 1;
    if (!h || (ftype != CSDR_FIRFILT_ARKAISER && ftype != CSDR_FIRFILT_RRC) || k < 2 || m < 1 || n > RNYQUIST_MAX_LEN ||
        !(beta > 0.f && beta <= 1.f) || !(dt >= -1.f && dt <= 1.f)) {
        set_error("firdes_rnyquist: bad arguments (ftype ARKAISER 7 or RRC 9, k >= 2, m >= 1, 2 k m + 1 <= %u, beta in (0, 1], dt in [-1, 1], h)",
                  RNYQUIST_MAX_LEN);
        return CSDR_ERR_INVALID;
    }
    const std::vector<float> t = design_rnyquist(ftype, k, m, beta, dt);
    if (t.empty()) {
        set_error("firdes_rnyquist: the ARKAISER bandwidth factor rho_hat of (m = %u, beta = %g) lies outside (0, 1)", m, (double)beta);
        return CSDR_ERR_INVALID;
    }
    std::memcpy(h, t.data(), sizeof(float) * t.size());
    return CSDR_OK;
}
int csdr_fir_groupdelay(const float *h, uint32_t n, float fc, float *gd)
{
    if (!h || !gd || !n || !(fc >= -0.5f && fc <= 0.5f)) { set_error("fir_groupdelay: bad arguments (n >= 1, |fc| <= 0.5)"); return CSDR_ERR_INVALID; }
    *gd = fir_group_delay(std::vector<float>(h, h + n), fc);
    return CSDR_OK;
}
}  // extern "C"
struct csdr_firfilt {
    int device; DeviceBuffers mem; uint32_t C, max_n, el; bool cplx; std::vector<float> taps; float scale;   // el: bytes per sample
    float *d_h = nullptr; PingPong<char> hist;                                             // hist: [C][L - 1] samples, in bytes
    char *d_x = nullptr, *d_y = nullptr;
    size_t hist_bytes() const { return (size_t)C * (taps.size() - 1) * el; }
};
extern "C" {
int csdr_firfilt_destroy(csdr_firfilt *h) { return block_destroy(h); }
int csdr_firfilt_create_taps(const float *taps, uint32_t n, float scale, int32_t is_complex, uint32_t nchan, uint32_t max_samples,
                             csdr_firfilt **out)
{
    if (!out || !taps || !nchan || n < 1 || n > FIRFILT_MAX_LEN || max_samples > (1u << 30)) {
        set_error("firfilt: bad arguments (taps, 1 <= n <= %u, nchan >= 1, max_samples <= 2^30)", FIRFILT_MAX_LEN);
        return CSDR_ERR_INVALID;
    }
    NewBlock<csdr_firfilt> h;
    int r = h.open(); if (r) return r;
    h->C = nchan; h->max_n = block_max_n(max_samples); h->cplx = is_complex != 0;
    h->el = h->cplx ? sizeof(float2) : sizeof(float);
    h->taps.assign(taps, taps + n); h->scale = scale;
    const size_t plane = (size_t)nchan * h->max_n * h->el;
    if ((r = block_upload(h->mem, &h->d_h, taps, n)) || (r = h->hist.alloc_zeroed(h->mem, h->hist_bytes())) ||
        (r = h->mem.alloc_n(&h->d_x, plane)) || (r = h->mem.alloc_n(&h->d_y, plane))) return r;
    return h.publish(out);
}
int csdr_firfilt_create_kaiser(uint32_t n, float fc, float as_db, float mu, int32_t is_complex, uint32_t nchan, uint32_t max_samples,
                               csdr_firfilt **out)
{
    if (!firdes_kaiser_args_ok(n, fc, as_db, mu)) {
        set_error("firfilt: bad design (n in [2, %u], fc in (0, 0.5], As > 0, mu == 0)", FIRFILT_MAX_LEN);
        return CSDR_ERR_INVALID;
    }
    const std::vector<float> t = design_firfilt_kaiser(n, fc, as_db);
    return csdr_firfilt_create_taps(t.data(), n, 2.0f * fc, is_complex, nchan, max_samples, out);   // firfilt_crcf_set_scale (2 fc), :893
}
int csdr_firfilt_process_device(csdr_firfilt *h, const void *d_x, uint32_t n, void *d_y, void *stream)
{
    if (!h) return block_null_arg("firfilt");
    if (int r = block_check_n("firfilt", n, h->max_n)) return r;
    if (!n) return CSDR_OK;
    if (!d_x || !d_y || d_x == d_y) { set_error("firfilt: null or aliased buffer"); return CSDR_ERR_INVALID; }
    const FirfiltLaunch l{h->C, n, (uint32_t)h->taps.size(), h->scale};
    return h->hist.flip_behind(launch_firfilt(h->cplx, d_x, d_y, h->d_h, h->hist.in(), h->hist.out(), l, (hipStream_t)stream));
}
int csdr_firfilt_process(csdr_firfilt *h, const float *x, uint32_t n, float *y)
{
    if (int r = block_check_call("firfilt", h, x, n, y)) return r;
    if (!n) return CSDR_OK;
    const size_t bytes = (size_t)h->C * n * h->el;
    return block_round_trip("firfilt", h->device, h->d_x, x, bytes, h->d_y, y, bytes,
                            [&] { return csdr_firfilt_process_device(h, h->d_x, n, h->d_y, nullptr); });
}
int csdr_firfilt_reset(csdr_firfilt *h) { return block_reset(h, [&] { return h->hist.reset(nullptr); }); }
uint32_t csdr_firfilt_get_taps_len(const csdr_firfilt *h) { return h ? (uint32_t)h->taps.size() : 0; }
int csdr_firfilt_get_taps(const csdr_firfilt *h, float *taps, float *scale)
{
    if (!h) return CSDR_ERR_INVALID;
    if (taps) std::memcpy(taps, h->taps.data(), sizeof(float) * h->taps.size());
    if (scale) *scale = h->scale;
    return CSDR_OK;
}

// ---------------------------------------------------------------------------
// gmskDemodulator m k bw (Liquid.chs:384-429): gmskdem on nchan independent CF32 streams; the two design
// functions need no GPU
// ---------------------------------------------------------------------------
static int firdes_gmsk(const char *name, bool rx, uint32_t k, uint32_t m, float bt, float *h)
{
    if (!h || !gmsk_args_ok(k, m, bt)) {
        set_error("%s: bad arguments (k in [%u, %u], m in [1, %u], BT in [0.2, 1], h)", name, GMSK_MIN_K, GMSK_MAX_K, GMSK_MAX_M);
        return CSDR_ERR_INVALID;
    }
    const std::vector<float> t = rx ? design_gmskrx(k, m, bt) : design_gmsktx(k, m, bt);
    std::memcpy(h, t.data(), sizeof(float) * t.size());
    return CSDR_OK;
}
int csdr_firdes_gmsktx(uint32_t k, uint32_t m, float bt, float *h) { return firdes_gmsk("firdes_gmsktx", false, k, m, bt, h); }
int csdr_firdes_gmskrx(uint32_t k, uint32_t m, float bt, float *h) { return firdes_gmsk("firdes_gmskrx", true, k, m, bt, h); }
}  // extern "C"
struct csdr_gmskdem {
    int device; DeviceBuffers mem; uint32_t C, max_n, k, m; std::vector<float> taps;
    float *d_h = nullptr; PingPong<float2> hist;                                           // hist: [C][L] samples
    float2 *d_x = nullptr; uint32_t *d_sym = nullptr;
    float *d_soft = nullptr;                                // host-path soft values: allocated by the first call that asks for them
};
extern "C" {
int csdr_gmskdem_destroy(csdr_gmskdem *h) { return block_destroy(h); }
int csdr_gmskdem_create(uint32_t k, uint32_t m, float bt, uint32_t nchan, uint32_t max_samples, csdr_gmskdem **out)
{
    if (!out || !nchan || !gmsk_args_ok(k, m, bt) || max_samples > (1u << 30)) {
        set_error("gmskdem: bad arguments (k in [%u, %u], m in [1, %u], BT in [0.2, 1], nchan >= 1, max_samples <= 2^30)", GMSK_MIN_K,
                  GMSK_MAX_K, GMSK_MAX_M);
        return CSDR_ERR_INVALID;
    }
    NewBlock<csdr_gmskdem> h;
    int r = h.open(); if (r) return r;
    h->C = nchan; h->max_n = block_max_n(max_samples); h->k = k; h->m = m;
    h->taps = design_gmskrx(k, m, bt);
    const size_t C = nchan, n = h->max_n, L = h->taps.size();
    if ((r = block_upload(h->mem, &h->d_h, h->taps.data(), L)) || (r = h->hist.alloc_zeroed(h->mem, C * L)) ||
        (r = h->mem.alloc_n(&h->d_x, C * n)) || (r = h->mem.alloc_n(&h->d_sym, C * (n / k) + 1))) return r;
    return h.publish(out);
}
// n has to be a multiple of k (the reference throws, Liquid.chs:421) and at most max_samples; nothing is touched otherwise
static int gmskdem_check_n(const csdr_gmskdem *h, uint32_t n)
{
    if (n % h->k) { set_error("gmskdem: %u samples are not a multiple of k = %u", n, h->k); return CSDR_ERR_SIZE; }
    return block_check_n("gmskdem", n, h->max_n);
}
int csdr_gmskdem_process_device(csdr_gmskdem *h, const void *d_x, uint32_t n, void *d_sym, void *d_soft, void *stream)
{
    if (!h) return block_null_arg("gmskdem");
    int r = gmskdem_check_n(h, n); if (r) return r;
    if (!n) return CSDR_OK;
    if (!d_x || !d_sym) { set_error("gmskdem: null buffer"); return CSDR_ERR_INVALID; }
    const GmskdemLaunch l{h->C, n, h->k, h->m, (uint32_t)h->taps.size(), (uint32_t)(0x100000000ull / h->k) + 1u};
    return h->hist.flip_behind(launch_gmskdem((const float2 *)d_x, (uint32_t *)d_sym, (float *)d_soft, h->d_h, h->hist.in(), h->hist.out(), l,
                                              (hipStream_t)stream));
}
int csdr_gmskdem_process(csdr_gmskdem *h, const float *x, uint32_t n, uint32_t *sym, float *soft, uint32_t *n_out)
{
    if (!h || !n_out) return block_null_arg("gmskdem");
    int r = gmskdem_check_n(h, n); if (r) return r;
    const size_t ns = n / h->k, C = h->C;
    *n_out = (uint32_t)(C * ns);
    if (!n) return CSDR_OK;
    if (!x || !sym) { set_error("gmskdem: null buffer"); return CSDR_ERR_INVALID; }
    if (soft && (r = block_lazy_alloc("gmskdem", h->device, h->mem, &h->d_soft, C * (h->max_n / h->k) + 1))) return r;
    return block_host_call("gmskdem", h->device, h->d_x, x, sizeof(float2) * C * n,
                           [&] { return csdr_gmskdem_process_device(h, h->d_x, n, h->d_sym, soft ? h->d_soft : nullptr, nullptr); },
                           {{sym, h->d_sym, sizeof(uint32_t) * C * ns}, {soft, h->d_soft, sizeof(float) * C * ns}});
}
int csdr_gmskdem_reset(csdr_gmskdem *h) { return block_reset(h, [&] { return h->hist.reset(nullptr); }); }
int csdr_gmskdem_get_design(const csdr_gmskdem *h, uint32_t *taps_len, float *taps)
{
    if (!h) return block_null_arg("gmskdem");
    if (taps_len) *taps_len = (uint32_t)h->taps.size();
    if (taps) std::memcpy(taps, h->taps.data(), sizeof(float) * h->taps.size());
    return CSDR_OK;
}

// ---------------------------------------------------------------------------
// iirCFilter n fc f0 ap as (Liquid.chs:594-608) and its F32 and bring-your-own-sections forms: a cascade of second-order
// sections on nchan independent rows; the design function needs no GPU
// ---------------------------------------------------------------------------
static bool iirdes_args_ok(uint32_t order, float fc) { return order >= 1 && order <= IIRSOS_MAX_ORDER && fc > 0.f && fc < 0.5f; }
int csdr_iirdes_butter_lowpass(uint32_t order, float fc, float *b, float *a)
{
    if (!b || !a || !iirdes_args_ok(order, fc)) {
        set_error("iirdes_butter_lowpass: bad arguments (order in [1, %u], fc in (0, 0.5))", IIRSOS_MAX_ORDER);
        return CSDR_ERR_INVALID;
    }
    design_butter_lowpass_sos(order, fc, b, a);
    return CSDR_OK;
}
}  // extern "C"
struct csdr_iirsos {
    int device; DeviceBuffers mem; uint32_t C, max_n, el; bool cplx; std::vector<float> b, a;   // el: bytes per sample; b, a [3 S], a0 = 1
    IirSosSection *d_sec = nullptr; char *d_st = nullptr, *d_x = nullptr, *d_y = nullptr;  // d_st [C][S] states of 2 samples, in place
    uint32_t nsec() const { return (uint32_t)(b.size() / 3); }
    size_t st_bytes() const { return (size_t)C * nsec() * 2 * el; }
};
extern "C" {
int csdr_iirsos_destroy(csdr_iirsos *h) { return block_destroy(h); }
int csdr_iirsos_create_sos(const float *b, const float *a, uint32_t nsec, int32_t is_complex, uint32_t nchan, uint32_t max_samples,
                           csdr_iirsos **out)
{
    if (!out || !b || !a || !nchan || nsec < 1 || nsec > IIRSOS_MAX_SEC || max_samples > (1u << 30)) {
        set_error("iirsos: bad arguments (b, a, 1 <= nsec <= %u, nchan >= 1, max_samples <= 2^30)", IIRSOS_MAX_SEC);
        return CSDR_ERR_INVALID;
    }
    // every section divided by its a0 (iirfiltsos), then strictly stable: the scan's matrix powers would overflow otherwise
    std::vector<float> bn(3 * nsec), an(3 * nsec);
    std::vector<IirSosSection> sec(nsec);
    for (uint32_t s = 0; s < nsec; s++) {
        const float a0 = a[3 * s];
        if (!(a0 != 0.f) || !std::isfinite(a0)) { set_error("iirsos: section %u has a0 = %g", s, (double)a0); return CSDR_ERR_INVALID; }
        for (int i = 0; i < 3; i++) { bn[3 * s + i] = b[3 * s + i] / a0; an[3 * s + i] = a[3 * s + i] / a0; }
        an[3 * s] = 1.f;
        const double a1 = an[3 * s + 1], a2 = an[3 * s + 2];
        const bool finite = std::isfinite(bn[3 * s]) && std::isfinite(bn[3 * s + 1]) && std::isfinite(bn[3 * s + 2]);
        if (!finite || !(std::fabs(a2) < 1.0) || !(std::fabs(a1) < 1.0 + a2)) {
            set_error("iirsos: section %u is not strictly stable or not finite (needs |a2| < 1 and |a1| < 1 + a2; a1 = %g, a2 = %g)", s, a1, a2);
            return CSDR_ERR_INVALID;
        }
        sec[s] = make_iirsos_section(&bn[3 * s], an[3 * s + 1], an[3 * s + 2]);
    }
    NewBlock<csdr_iirsos> h;
    int r = h.open(); if (r) return r;
    h->C = nchan; h->max_n = block_max_n(max_samples); h->cplx = is_complex != 0;
    h->el = h->cplx ? sizeof(float2) : sizeof(float);
    h->b = bn; h->a = an;
    const size_t plane = (size_t)nchan * h->max_n * h->el;
    if ((r = block_upload(h->mem, &h->d_sec, sec.data(), nsec)) || (r = block_zeros(h->mem, &h->d_st, h->st_bytes())) ||
        (r = h->mem.alloc_n(&h->d_x, plane)) || (r = h->mem.alloc_n(&h->d_y, plane))) return r;
    return h.publish(out);
}
int csdr_iirsos_create_prototype(uint32_t order, float fc, float f0, float ap, float as_db, int32_t is_complex, uint32_t nchan,
                                 uint32_t max_samples, csdr_iirsos **out)
{
    (void)f0; (void)ap; (void)as_db;              // do not enter a Butterworth low-pass; ignored, as csdr_iirfilt_create does
    if (!iirdes_args_ok(order, fc)) {
        set_error("iirsos: bad design (order in [1, %u], fc in (0, 0.5))", IIRSOS_MAX_ORDER);
        return CSDR_ERR_INVALID;
    }
    const uint32_t S = (order + 1) / 2;
    float b[3 * IIRSOS_MAX_SEC], a[3 * IIRSOS_MAX_SEC];
    design_butter_lowpass_sos(order, fc, b, a);
    return csdr_iirsos_create_sos(b, a, S, is_complex, nchan, max_samples, out);
}
int csdr_iirsos_process_device(csdr_iirsos *h, const void *d_x, uint32_t n, void *d_y, void *stream)
{
    if (!h) return block_null_arg("iirsos");
    if (int r = block_check_n("iirsos", n, h->max_n)) return r;
    if (!n) return CSDR_OK;
    if (!d_x || !d_y) { set_error("iirsos: null buffer"); return CSDR_ERR_INVALID; }
    return launch_iirsos(h->cplx, d_x, d_y, h->C, n, h->nsec(), h->d_sec, h->d_st, (hipStream_t)stream);
}
int csdr_iirsos_process(csdr_iirsos *h, const float *x, uint32_t n, float *y)
{
    if (int r = block_check_call("iirsos", h, x, n, y)) return r;
    if (!n) return CSDR_OK;
    const size_t bytes = (size_t)h->C * n * h->el;
    return block_round_trip("iirsos", h->device, h->d_x, x, bytes, h->d_y, y, bytes,
                            [&] { return csdr_iirsos_process_device(h, h->d_x, n, h->d_y, nullptr); });
}
int csdr_iirsos_reset(csdr_iirsos *h)
{
    return block_reset(h, [&] { CSDR_HIP(hipMemset(h->d_st, 0, h->st_bytes())); return (int)CSDR_OK; });
}
uint32_t csdr_iirsos_get_nsec(const csdr_iirsos *h) { return h ? h->nsec() : 0; }
int csdr_iirsos_get_sos(const csdr_iirsos *h, float *b, float *a)
{
    if (!h) return CSDR_ERR_INVALID;
    if (b) std::memcpy(b, h->b.data(), sizeof(float) * h->b.size());
    if (a) std::memcpy(a, h->a.data(), sizeof(float) * h->a.size());
    return CSDR_OK;
}

// ---------------------------------------------------------------------------
// firpfbch2Channelizer: liquid's firpfbch2_crcf analyzer, which the reference does not import.  The constructors
// are `open` and the reset is `rewind`; the design and launch-shape functions need no GPU
// ---------------------------------------------------------------------------
}  // extern "C"
static bool pfbch2_design_args_ok(uint32_t M, uint32_t m, float as_db, float fc)
{
    return pfb2_args_ok(M, m) && std::isfinite(as_db) && as_db > 0.f && std::isfinite(fc) && fc >= 0.f && fc < 0.5f;
}
// what csdr_pfbch2 and csdr_pfbsyn2 (name) share: the refusal of a design, the argument check of open_taps, the six words of
// launch_shape (shape_of: pfb2_shape or pfb2s_shape) and get_taps
static int pfb2_bad_design(const char *name)
{
    set_error("%s: bad arguments (M a power of two in [%u, %u], m in [1, %u], As > 0, fc = 0 or in (0, 0.5), finite)", name, PFB2_MIN_M,
              PFB2_MAX_M, PFB2_MAX_SEMI);
    return CSDR_ERR_INVALID;
}
static int pfb2_check_open(const char *name, const void *out, const float *taps, uint32_t M, uint32_t m, uint32_t max_frames)
{
    bool ok = out && taps && pfb2_args_ok(M, m) && max_frames && (uint64_t)max_frames * M <= (1ull << 31);
    for (uint32_t i = 0; ok && i < 2 * M * m; i++) ok = std::isfinite(taps[i]);
    if (ok) return CSDR_OK;
    set_error("%s: bad arguments (finite taps, M a power of two in [%u, %u], m in [1, %u], 1 <= max_frames <= 2^31 / M)", name, PFB2_MIN_M,
              PFB2_MAX_M, PFB2_MAX_SEMI);
    return CSDR_ERR_INVALID;
}
static int pfb2_launch_shape(const char *name, Pfb2Shape (*shape_of)(uint32_t, uint32_t, uint32_t, uint32_t), uint32_t M, uint32_t m,
                             uint32_t frames, uint32_t cus, uint32_t *shape)
{
    if (!shape || !pfb2_args_ok(M, m) || !cus) { set_error("%s_launch_shape: bad arguments (M, m as for the block, cus >= 1, shape)", name); return CSDR_ERR_INVALID; }
    const Pfb2Shape s = shape_of(M, m, frames, cus);
    const uint32_t v[6] = {s.F, s.tiles, s.tiles_per_run, s.runs, s.wgs_per_cu, (uint32_t)s.lds};
    std::memcpy(shape, v, sizeof(v));
    return CSDR_OK;
}
template <class H> static int pfb2_get_taps(const char *name, const H *h, float *taps)
{
    if (!h || !taps) return block_null_arg(name);
    std::memcpy(taps, h->taps.data(), sizeof(float) * h->taps.size());
    return CSDR_OK;
}
extern "C" {
int csdr_pfbch2_design(uint32_t M, uint32_t m, float as_db, float fc, float *h)
{
    if (!h || !pfbch2_design_args_ok(M, m, as_db, fc)) return pfb2_bad_design("pfbch2");
    const std::vector<float> t = design_pfb2_taps(M, m, as_db, fc);
    std::memcpy(h, t.data(), sizeof(float) * 2 * M * m);
    return CSDR_OK;
}
int csdr_pfbch2_launch_shape(uint32_t M, uint32_t m, uint32_t frames, uint32_t cus, uint32_t *shape)
{
    return pfb2_launch_shape("pfbch2", pfb2_shape, M, m, frames, cus, shape);
}
}  // extern "C"
struct csdr_pfbch2 {
    int device; DeviceBuffers mem; uint32_t M, m, max_n, max_frames, cus, parity = 0; std::vector<float> taps;    // max_n: samples per call
    float *d_h = nullptr; float2 *d_tw = nullptr, *d_x = nullptr, *d_y = nullptr; PingPong<float2> hist;           // hist: [2 m M - M / 2]
};
extern "C" {
int csdr_pfbch2_destroy(csdr_pfbch2 *h) { return block_destroy(h); }
int csdr_pfbch2_open_taps(const float *taps, uint32_t M, uint32_t m, uint32_t max_frames, csdr_pfbch2 **out)
{
    int r = pfb2_check_open("pfbch2", out, taps, M, m, max_frames); if (r) return r;
    NewBlock<csdr_pfbch2> h;
    if ((r = h.open())) return r;
    h->M = M; h->m = m; h->max_frames = max_frames; h->max_n = max_frames * (M / 2); h->cus = block_cu_count(h->device);
    h->taps.assign(taps, taps + 2 * M * m);
    const std::vector<float2> tw = pfb2_twiddles(M);
    if ((r = block_upload(h->mem, &h->d_h, taps, h->taps.size())) || (r = block_upload(h->mem, &h->d_tw, tw.data(), tw.size())) ||
        (r = h->hist.alloc_zeroed(h->mem, h->taps.size() - M / 2)) || (r = h->mem.alloc_n(&h->d_x, (size_t)h->max_n)) ||
        (r = h->mem.alloc_n(&h->d_y, (size_t)max_frames * M))) return r;
    return h.publish(out);
}
int csdr_pfbch2_open_kaiser(uint32_t M, uint32_t m, float as_db, float fc, uint32_t max_frames, csdr_pfbch2 **out)
{
    if (!pfbch2_design_args_ok(M, m, as_db, fc)) return pfb2_bad_design("pfbch2");
    const std::vector<float> t = design_pfb2_taps(M, m, as_db, fc);
    return csdr_pfbch2_open_taps(t.data(), M, m, max_frames, out);
}
// n has to be a whole number of frames of M / 2 samples, at most max_frames of them; nothing is touched otherwise
static int pfbch2_check_n(const csdr_pfbch2 *h, uint32_t n)
{
    if (n % (h->M / 2)) { set_error("pfbch2: %u samples are not a multiple of M / 2 = %u", n, h->M / 2); return CSDR_ERR_SIZE; }
    return block_check_n("pfbch2", n, h->max_n);
}
int csdr_pfbch2_process_device(csdr_pfbch2 *h, const void *d_x, uint32_t n, void *d_y, void *stream)
{
    if (!h) return block_null_arg("pfbch2");
    if (int r = pfbch2_check_n(h, n)) return r;
    if (!n) return CSDR_OK;
    if (!d_x || !d_y || d_x == d_y) { set_error("pfbch2: null or aliased buffer"); return CSDR_ERR_INVALID; }
    const uint32_t frames = n / (h->M / 2);
    const int r = launch_pfb2((const float2 *)d_x, (float2 *)d_y, h->d_h, h->d_tw, h->hist.in(), h->hist.out(), h->M, h->m, frames, h->parity,
                              h->cus, (hipStream_t)stream);
    if (!r) { h->hist.flip(); h->parity = (h->parity + frames) & 1u; }
    return r;
}
int csdr_pfbch2_process(csdr_pfbch2 *h, const float *x, uint32_t n, float *y, uint32_t *frames)
{
    if (!frames) return block_null_arg("pfbch2");
    if (int r = block_check_call("pfbch2", h, x, n, y)) return r;
    if (int r = pfbch2_check_n(h, n)) return r;
    *frames = n / (h->M / 2);
    if (!n) return CSDR_OK;
    return block_round_trip("pfbch2", h->device, h->d_x, x, sizeof(float2) * n, h->d_y, y, sizeof(float2) * *frames * h->M,
                            [&] { return csdr_pfbch2_process_device(h, h->d_x, n, h->d_y, nullptr); });
}
int csdr_pfbch2_rewind(csdr_pfbch2 *h)
{
    return block_reset(h, [&] { const int r = h->hist.reset(nullptr); if (!r) h->parity = 0; return r; });
}
int csdr_pfbch2_get_taps(const csdr_pfbch2 *h, float *taps) { return pfb2_get_taps("pfbch2", h, taps); }

// ---------------------------------------------------------------------------
// firpfbch2Synthesizer: the synthesizer side of liquid's firpfbch2_crcf, the way back from csdr_pfbch2's rows.
// Names as csdr_pfbch2's: `open` and `rewind`; the design and launch-shape functions need no GPU
// ---------------------------------------------------------------------------
// design_pfb2_taps with the synthesizer's rule for fc = 0: 0.5 / M, half the analyzer's cutoff
static std::vector<float> pfbsyn2_taps(uint32_t M, uint32_t m, float as_db, float fc)
{
    return design_pfb2_taps(M, m, as_db, fc == 0.f ? 0.5f / (float)M : fc);
}
int csdr_pfbsyn2_design(uint32_t M, uint32_t m, float as_db, float fc, float *g)
{
    if (!g || !pfbch2_design_args_ok(M, m, as_db, fc)) return pfb2_bad_design("pfbsyn2");
    const std::vector<float> t = pfbsyn2_taps(M, m, as_db, fc);
    std::memcpy(g, t.data(), sizeof(float) * 2 * M * m);
    return CSDR_OK;
}
int csdr_pfbsyn2_launch_shape(uint32_t M, uint32_t m, uint32_t frames, uint32_t cus, uint32_t *shape)
{
    return pfb2_launch_shape("pfbsyn2", pfb2s_shape, M, m, frames, cus, shape);
}
}  // extern "C"
struct csdr_pfbsyn2 {
    int device; DeviceBuffers mem; uint32_t M, m, max_n, cus, parity = 0, seen = 0; std::vector<float> taps;   // max_n: frames per call
    float *d_g = nullptr; float2 *d_tw = nullptr, *d_y = nullptr, *d_x = nullptr; PingPong<float2> hist;         // hist: [M][4 m - 1]
};
extern "C" {
int csdr_pfbsyn2_destroy(csdr_pfbsyn2 *h) { return block_destroy(h); }
int csdr_pfbsyn2_open_taps(const float *taps, uint32_t M, uint32_t m, uint32_t max_frames, csdr_pfbsyn2 **out)
{
    int r = pfb2_check_open("pfbsyn2", out, taps, M, m, max_frames); if (r) return r;
    NewBlock<csdr_pfbsyn2> h;
    if ((r = h.open())) return r;
    h->M = M; h->m = m; h->max_n = max_frames; h->cus = block_cu_count(h->device);
    h->taps.assign(taps, taps + 2 * M * m);
    const std::vector<float2> tw = pfb2_twiddles(M);
    if ((r = block_upload(h->mem, &h->d_g, taps, h->taps.size())) || (r = block_upload(h->mem, &h->d_tw, tw.data(), tw.size())) ||
        (r = h->hist.alloc_zeroed(h->mem, (size_t)M * pfb2s_halo_frames(m))) || (r = h->mem.alloc_n(&h->d_y, (size_t)max_frames * M)) ||
        (r = h->mem.alloc_n(&h->d_x, (size_t)max_frames * (M / 2)))) return r;
    return h.publish(out);
}
int csdr_pfbsyn2_open_kaiser(uint32_t M, uint32_t m, float as_db, float fc, uint32_t max_frames, csdr_pfbsyn2 **out)
{
    if (!pfbch2_design_args_ok(M, m, as_db, fc)) return pfb2_bad_design("pfbsyn2");
    const std::vector<float> t = pfbsyn2_taps(M, m, as_db, fc);
    return csdr_pfbsyn2_open_taps(t.data(), M, m, max_frames, out);
}
int csdr_pfbsyn2_process_device(csdr_pfbsyn2 *h, const void *d_y, uint32_t frames, void *d_x, void *stream)
{
    if (!h) return block_null_arg("pfbsyn2");
    if (int r = block_check_n("pfbsyn2", frames, h->max_n)) return r;
    if (!frames) return CSDR_OK;
    if (!d_y || !d_x || d_y == d_x) { set_error("pfbsyn2: null or aliased buffer"); return CSDR_ERR_INVALID; }
    const int r = launch_pfb2s((const float2 *)d_y, (float2 *)d_x, h->d_g, h->d_tw, h->hist.in(), h->hist.out(), h->M, h->m, frames, h->parity,
                               h->seen, h->cus, (hipStream_t)stream);
    if (!r) {
        h->hist.flip();
        h->parity = (h->parity + frames) & 1u;
        h->seen = (uint32_t)std::min<uint64_t>((uint64_t)h->seen + frames, pfb2s_halo_frames(h->m));
    }
    return r;
}
int csdr_pfbsyn2_process(csdr_pfbsyn2 *h, const float *y, uint32_t frames, float *x, uint32_t *n)
{
    if (!n) return block_null_arg("pfbsyn2");
    if (int r = block_check_call("pfbsyn2", h, y, frames, x)) return r;
    if (frames && (const void *)y == (const void *)x) { set_error("pfbsyn2: aliased buffer"); return CSDR_ERR_INVALID; }
    *n = frames * (h->M / 2);
    if (!frames) return CSDR_OK;
    return block_round_trip("pfbsyn2", h->device, h->d_y, y, sizeof(float2) * frames * h->M, h->d_x, x, sizeof(float2) * *n,
                            [&] { return csdr_pfbsyn2_process_device(h, h->d_y, frames, h->d_x, nullptr); });
}
int csdr_pfbsyn2_rewind(csdr_pfbsyn2 *h)
{
    return block_reset(h, [&] { const int r = h->hist.reset(nullptr); if (!r) h->parity = h->seen = 0; return r; });
}
int csdr_pfbsyn2_get_taps(const csdr_pfbsyn2 *h, float *taps) { return pfb2_get_taps("pfbsyn2", h, taps); }
uint32_t csdr_pfbsyn2_delay(const csdr_pfbsyn2 *h) { return h ? 2 * h->M * h->m - h->M / 2 + 1 : 0; }

// ---------------------------------------------------------------------------
// rowResampler: liquid's resamp_crcf / resamp_rrrf on nchan rows, which the reference does not import ("csdr rowresamp v1",
// DESIGN.md 4.19).  Names as csdr_pfbch2's: `open` and `rewind`; the design and launch-shape functions need no GPU
// ---------------------------------------------------------------------------
static int rowresamp_bad_design()
{
    set_error("rowresamp: bad arguments (1/8 <= rate <= 8, m in [1, %u] with m D <= %u, 0 < as <= 120, fc = 0 or in (0, 0.5))", RRS_MAX_SEMI,
              RRS_MAX_SEMI_D);
    return CSDR_ERR_INVALID;
}
int csdr_rowresamp_design(double rate, uint32_t m, float as_db, float fc, uint32_t *taps_per_phase, uint64_t *delta, float *bank)
{
    if (!rowresamp_design_args_ok(rate, m, as_db, fc)) return rowresamp_bad_design();
    const RowResampDesign d = design_rowresamp(rate, m, as_db, fc);
    if (taps_per_phase) *taps_per_phase = d.P;
    if (delta) *delta = d.delta;
    if (bank) std::memcpy(bank, d.bank.data(), sizeof(float) * d.bank.size());
    return CSDR_OK;
}
int csdr_rowresamp_launch_shape(double rate, uint32_t m, int32_t is_complex, uint32_t n_out, uint32_t nchan, uint32_t cus, uint64_t t_next,
                                uint32_t *shape)
{
    if (!shape || !rowresamp_design_args_ok(rate, m, 60.f, 0.f) || !nchan || !cus) {
        set_error("rowresamp_launch_shape: bad arguments (rate, m as for the block, nchan >= 1, cus >= 1, shape)");
        return CSDR_ERR_INVALID;
    }
    const uint64_t delta = (uint64_t)std::llround(4294967296.0 / rate);
    const RrsShape s = rrs_shape(delta, m, is_complex != 0, n_out, nchan, cus, t_next);
    if (!s.ok) { set_error("rowresamp_launch_shape: %u rows of %u outputs are too many tiles", nchan, n_out); return CSDR_ERR_SIZE; }
    const uint32_t v[8] = {s.P, s.TO, s.window, (uint32_t)s.lds, s.wgs_per_cu, s.tiles, s.items_per_run, s.runs};
    std::memcpy(shape, v, sizeof(v));
    return CSDR_OK;
}
}  // extern "C"
struct csdr_rowresamp {
    int device; DeviceBuffers mem; uint32_t m, nchan, max_n, cus; bool cplx; uint64_t delta, T = 0; RowResampDesign design;
    float *d_bank = nullptr; float *d_x = nullptr, *d_y = nullptr; PingPong<float> hist;    // d_bank: [P][RRS_BANK_STRIDE]; hist: [nchan][P - 1] samples
    size_t elem() const { return cplx ? 2 : 1; }                                             // floats per sample
    uint32_t max_out(uint32_t n) const { return rrs_count(0, delta, n); }
};
extern "C" {
int csdr_rowresamp_destroy(csdr_rowresamp *h) { return block_destroy(h); }
int csdr_rowresamp_open(double rate, uint32_t m, float as_db, float fc, int32_t is_complex, uint32_t nchan, uint32_t max_samples,
                        csdr_rowresamp **out)
{
    if (!rowresamp_design_args_ok(rate, m, as_db, fc)) return rowresamp_bad_design();
    if (!out || !nchan || !max_samples || max_samples > (1u << 28)) {
        set_error("rowresamp: bad arguments (nchan >= 1, 1 <= max_samples <= 2^28, out)");
        return CSDR_ERR_INVALID;
    }
    NewBlock<csdr_rowresamp> h;
    int r = h.open(); if (r) return r;
    h->design = design_rowresamp(rate, m, as_db, fc);
    h->m = m; h->nchan = nchan; h->max_n = max_samples; h->cus = block_cu_count(h->device); h->cplx = is_complex != 0; h->delta = h->design.delta;
    const uint32_t P = h->design.P;
    std::vector<float> bank_t((size_t)RRS_BANK_STRIDE * P, 0.f);                             // the kernel's [j][column(b)] image
    for (uint32_t b = 0; b <= RRS_NPFB; b++)
        for (uint32_t j = 0; j < P; j++) bank_t[(size_t)j * RRS_BANK_STRIDE + rrs_bank_col(b)] = h->design.bank[(size_t)b * P + j];
    if ((r = block_upload(h->mem, &h->d_bank, bank_t.data(), bank_t.size())) ||
        (r = h->hist.alloc_zeroed(h->mem, (size_t)nchan * (P - 1) * h->elem())) ||
        (r = h->mem.alloc_n(&h->d_x, (size_t)nchan * max_samples * h->elem())) ||
        (r = h->mem.alloc_n(&h->d_y, (size_t)nchan * h->max_out(max_samples) * h->elem()))) return r;
    return h.publish(out);
}
uint32_t csdr_rowresamp_max_out(const csdr_rowresamp *h, uint32_t n) { return h && n <= h->max_n ? h->max_out(n) : 0; }
int csdr_rowresamp_count(const csdr_rowresamp *h, uint32_t n, uint32_t *n_out)
{
    if (!h || !n_out) return block_null_arg("rowresamp");
    if (int r = block_check_n("rowresamp", n, h->max_n)) return r;
    *n_out = rrs_count(h->T, h->delta, n);
    return CSDR_OK;
}
int csdr_rowresamp_process_device(csdr_rowresamp *h, const void *d_x, uint32_t n, void *d_y, uint32_t *n_out, void *stream)
{
    if (!h || !n_out) return block_null_arg("rowresamp");
    if (int r = block_check_n("rowresamp", n, h->max_n)) return r;
    if (!n) { *n_out = 0; return CSDR_OK; }
    if (!d_x || !d_y || d_x == d_y) { set_error("rowresamp: null or aliased buffer"); return CSDR_ERR_INVALID; }
    const uint32_t cnt = rrs_count(h->T, h->delta, n);
    const int r = launch_rowresamp(d_x, d_y, h->d_bank, h->hist.in(), h->hist.out(), h->delta, h->m, h->cplx, h->nchan, n, cnt, h->T, h->cus,
                                   (hipStream_t)stream);
    if (r) return r;
    h->hist.flip();
    h->T = rrs_next_time(h->T, h->delta, n, cnt);
    *n_out = cnt;
    return CSDR_OK;
}
int csdr_rowresamp_process(csdr_rowresamp *h, const float *x, uint32_t n, float *y, uint32_t *n_out)
{
    if (!n_out) return block_null_arg("rowresamp");
    if (int r = block_check_call("rowresamp", h, x, n, y)) return r;
    if (n && (const void *)x == (const void *)y) { set_error("rowresamp: aliased buffer"); return CSDR_ERR_INVALID; }
    if (!n) { *n_out = 0; return CSDR_OK; }
    const size_t sample = sizeof(float) * h->elem();
    const uint32_t cnt = rrs_count(h->T, h->delta, n);
    return block_round_trip("rowresamp", h->device, h->d_x, x, sample * h->nchan * n, h->d_y, y, sample * h->nchan * cnt,
                            [&] { return csdr_rowresamp_process_device(h, h->d_x, n, h->d_y, n_out, nullptr); });
}
int csdr_rowresamp_rewind(csdr_rowresamp *h)
{
    return block_reset(h, [&] { const int r = h->hist.reset(nullptr); if (!r) h->T = 0; return r; });
}
int csdr_rowresamp_get_design(const csdr_rowresamp *h, uint32_t *taps_per_phase, uint64_t *delta, uint32_t *delay, float *bank)
{
    if (!h) return block_null_arg("rowresamp");
    if (taps_per_phase) *taps_per_phase = h->design.P;
    if (delta) *delta = h->delta;
    if (delay) *delay = h->design.P / 2;
    if (bank) std::memcpy(bank, h->design.bank.data(), sizeof(float) * h->design.bank.size());
    return CSDR_OK;
}
int csdr_rowresamp_get_time(const csdr_rowresamp *h, uint64_t *t_next)
{
    if (!h || !t_next) return block_null_arg("rowresamp");
    *t_next = h->T;
    return CSDR_OK;
}

// ---------------------------------------------------------------------------
// pskTracker (Liquid.chs:119-175 behind the symbol synchroniser): power normaliser, carrier PLL, T/2 equaliser and BPSK / QPSK
// decisions on nchan independent CF32 rows; csdr_sincos_word needs no GPU
// ---------------------------------------------------------------------------
int csdr_sincos_word(uint32_t w, float *s, float *c)
{
    if (!s || !c) return block_null_arg("sincos_word");
    psk_sincos_word(w, s, c);
    return CSDR_OK;
}
}  // extern "C"
struct csdr_psktrack {
    int device; DeviceBuffers mem; uint32_t C, max_n; PskLaunch l;
    PingPong<uint32_t> st;                                  // [C][psk_state_words(eq_len)]; all zeros is the state right after new
    float2 *d_x = nullptr, *d_y = nullptr; uint32_t *d_sym = nullptr, *d_nx = nullptr, *d_ny = nullptr;   // the host path's
};
static int psktrack_launch(csdr_psktrack *h, const void *d_x, uint32_t n, const void *d_nx, void *d_y, void *d_sym, void *d_ny, void *stream)
{
    PskLaunch l = h->l;
    l.n = n;
    return h->st.flip_behind(launch_psktrack((const float2 *)d_x, (const uint32_t *)d_nx, (float2 *)d_y, (uint32_t *)d_sym, (uint32_t *)d_ny,
                                             h->st.in(), h->st.out(), l, (hipStream_t)stream));
}
extern "C" {
int csdr_psktrack_destroy(csdr_psktrack *h) { return block_destroy(h); }
int csdr_psktrack_new(uint32_t bits, uint32_t sps, uint32_t phase, uint32_t eq_len, float eq_mu, uint32_t eq_mode, uint32_t eq_delay,
                      float pll_bw, float agc_bw, uint32_t nchan, uint32_t max_samples, csdr_psktrack **out)
{
    const bool eq_ok = eq_len == 0 || (sps == 2 && (eq_len & 1u) && eq_len >= 3 && eq_len <= PSK_MAX_EQ);
    if (!out || !nchan || bits < 1 || bits > 2 || sps < 1 || sps > 2 || phase > 1 || !eq_ok || !(eq_mu >= 0.f && eq_mu <= 1.f) ||
        eq_mode > CSDR_PSKTRACK_EQ_CM || !(pll_bw >= 0.f && pll_bw <= 1.f) || !(agc_bw >= 0.f && agc_bw <= 1.f) || max_samples > (1u << 28)) {
        set_error("psktrack: bad arguments (bits 1 or 2, sps 1 or 2, phase 0 or 1, eq_len 0 or odd in [3, %u] with sps 2, eq_mu, pll_bw and "
                  "agc_bw in [0, 1], eq_mode 0 or 1, nchan >= 1, max_samples <= 2^28)", PSK_MAX_EQ);
        return CSDR_ERR_INVALID;
    }
    NewBlock<csdr_psktrack> h;
    int r = h.open(); if (r) return r;
    h->C = nchan; h->max_n = block_max_n(max_samples);
    h->l = PskLaunch{nchan, 0, bits, sps, phase, eq_len, eq_mode, eq_delay, eq_mu, agc_bw, pll_bw, std::sqrt(pll_bw)};
    const size_t C = nchan, n = h->max_n;
    DeviceBuffers &mem = h->mem;
    if ((r = h->st.alloc_zeroed(mem, C * psk_state_words(eq_len))) || (r = mem.alloc_n(&h->d_x, C * n)) || (r = mem.alloc_n(&h->d_y, C * n)) ||
        (r = mem.alloc_n(&h->d_sym, C * n)) || (r = mem.alloc_n(&h->d_nx, C)) || (r = mem.alloc_n(&h->d_ny, C)))
        return r;
    return h.publish(out);
}
int csdr_psktrack_process_device(csdr_psktrack *h, const void *d_x, uint32_t n, const void *d_nx, void *d_y, void *d_sym, void *d_ny,
                                 void *stream)
{
    if (!h || !d_ny) return block_null_arg("psktrack");
    if (int r = block_check_n("psktrack", n, h->max_n)) return r;
    if (n && (!d_x || !d_y)) { set_error("psktrack: null buffer"); return CSDR_ERR_INVALID; }
    return psktrack_launch(h, d_x, n, d_nx, d_y, d_sym, d_ny, stream);
}
int csdr_psktrack_process(csdr_psktrack *h, const float *x, uint32_t n, const uint32_t *nx, float *y, uint32_t *sym, uint32_t *ny)
{
    if (!ny) return block_null_arg("psktrack");
    int r = block_check_call("psktrack", h, x, n, y); if (r) return r;
    const size_t C = h->C;
    if (nx)
        for (size_t c = 0; c < C; c++)
            if (nx[c] > n) { set_error("psktrack: row %zu holds %u samples > n = %u", c, nx[c], n); return CSDR_ERR_SIZE; }
    return block_host_call("psktrack", h->device, h->d_x, x, sizeof(float2) * C * n,
                           [&] {
                               if (nx) CSDR_HIP(hipMemcpy(h->d_nx, nx, sizeof(uint32_t) * C, hipMemcpyHostToDevice));
                               return psktrack_launch(h, h->d_x, n, nx ? h->d_nx : nullptr, h->d_y, sym ? h->d_sym : nullptr, h->d_ny, nullptr);
                           },
                           {{ny, h->d_ny, sizeof(uint32_t) * C}, {y, h->d_y, sizeof(float2) * C * n}, {sym, h->d_sym, sizeof(uint32_t) * C * n}});
}
int csdr_psktrack_restart(csdr_psktrack *h) { return block_reset(h, [&] { return h->st.reset(nullptr); }); }
int csdr_psktrack_get_state(csdr_psktrack *h, uint32_t chan, uint32_t *theta, uint32_t *freq, float *p, uint32_t *nsym, float *w)
{
    if (!h || chan >= h->C) { set_error("psktrack: bad channel"); return CSDR_ERR_INVALID; }
    DevGuard guard(h->device);
    const uint32_t L = h->l.L;
    std::vector<uint32_t> s(psk_state_words(L));
    CSDR_HIP(hipDeviceSynchronize());
    CSDR_HIP(hipMemcpy(s.data(), h->st.in() + (size_t)chan * s.size(), sizeof(uint32_t) * s.size(), hipMemcpyDeviceToHost));
    const bool live = s[0] != 0u;
    const float one = 1.f;
    if (theta) *theta = live ? s[2] : 0u;
    if (freq) *freq = live ? s[3] : 0u;
    if (p) std::memcpy(p, live ? (const void *)&s[1] : (const void *)&one, sizeof(float));
    if (nsym) *nsym = live ? s[5] : 0u;
    if (w) {
        if (live) std::memcpy(w, &s[PSK_HDR], sizeof(float) * 2 * L);
        else for (uint32_t i = 0; i < 2 * L; i++) w[i] = i + 1 == L ? 1.f : 0.f;
    }
    return CSDR_OK;
}
int csdr_psktrack_get_design(const csdr_psktrack *h, float *alpha, float *beta, uint32_t *eq_len, uint32_t *lds_bytes)
{
    if (!h) return block_null_arg("psktrack");
    if (alpha) *alpha = h->l.alpha;
    if (beta) *beta = h->l.beta;
    if (eq_len) *eq_len = h->l.L;
    if (lds_bytes) *lds_bytes = (uint32_t)psk_lds_bytes(h->l.L);
    return CSDR_OK;
}

}  // extern "C"

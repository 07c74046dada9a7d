// The tails behind the plan of a chain handle (capi.hip): the AGC tail, the AM and the WBFM tails, the backward handle's row
// reversal.  Each one owns its buffers (out of the handle's mem) and its stream state, and has three operations: setup() from the
// configuration (allocations, design, its piece of csdr_chain_path), reset() and run() for one call.  The handle has a tail or it
// has not.  The launch shape of the time-parallel AGC tail is agc_tail_shape.h's.  Local to the translation unit that
// includes it.
#pragma once
#include "capi_internal.h"
#include <optional>

namespace csdr {
namespace {
// Z[C][nf] (channel-major CF32) -> AGC + squelch [+ freqdem] [+ mix] -> out: the time-parallel verified tail (tm: Z tile-major), or
// with CSDR_FLAG_AGC_SEQUENTIAL one lane per channel in place on Z.  State: AGC {g, y2', mode, timer} + freqdem r' per row
struct AgcTail {
    // front: a plan writes Z (none: the caller's rows are Z); fused: that plan may write Z tile-major and its path says +agc; cus: compute
    // units of the handle's device
    int setup(DeviceBuffers &mem, const csdr_chain_cfg &cfg, uint32_t C_, uint32_t max_nf, bool front, bool fused, uint32_t cus)
    {
        const bool sequential = (cfg.flags & CSDR_FLAG_AGC_SEQUENTIAL) != 0;
        C = C_; prm = make_agc(cfg.agc_threshold_db);
        fm = cfg.demod == CSDR_DEMOD_FM; mixo = cfg.mix && cfg.channels > 1;
        if (fm) fm_ref = fm_ref_of(cfg.kf);
        in_place = front && sequential && !fm && !mixo;
        int r;
        if ((r = mem.alloc_n(&st, C))) return r;
        if (fm && (r = rp.alloc(mem, C))) return r;
        if (front || sequential) {      // (the one-lane-per-channel kernel works in place: on the caller's rows it needs a copy)
            // The fused plans may write the plane tile-major for k_agc_spec_tm, which reads up to a segment in front of / behind it.
            // The guards (2 x 64 KiB per channel: 128 MiB at 1024 channels) exist only where a call can take that route: a fused plan (the
            // any-M plan never writes tile-major), a time-parallel tail, a channel count k_agc_spec_tm takes, calls of >= 4 W = 4096 frames
            // 
            if (fused && !sequential && max_nf >= 4096u && agc_tail_tm_channels_ok(C)) guard = agc_tail_tm_guard(C);
            const size_t n = (size_t)C * max_nf;
            if ((r = mem.alloc_n(&d_A, n + 2 * guard))) return r;
            if (guard) {
                // only the guards need defined contents (the warm-ups of the first and last segments read them, masked by position)
                CSDR_HIP(hipMemset(d_A, 0, sizeof(float2) * guard));
                CSDR_HIP(hipMemset(d_A + guard + n, 0, sizeof(float2) * guard));
            }
        }
        if (mixo && (r = mem.alloc_n(&d_B, (size_t)C * max_nf))) return r;
        if (!sequential && (r = spec.emplace().init(mem, C, max_nf, cus))) return r;
        piece = !spec ? "" : (fused || !front) ? "-spec" : "+agc-spec";
        return CSDR_OK;
    }
    const char *path_piece() const { return piece; }        // the last piece of csdr_chain_path, behind the other tails'
    int reset(hipStream_t s)
    {
        int r = launch_agc_init(st, C, s); if (r) return r;
        if (spec) spec->reset();
        return fm ? rp.reset(s) : CSDR_OK;
    }
    bool time_parallel() const { return spec.has_value(); }         // (reads Z only)
    // where a front writes Z for run(..., out): the tail's plane, or out itself where the sequential AGC is the last step
    float2 *plane(void *out) const { return in_place ? (float2 *)out : d_A + guard; }
    bool tile_major(uint32_t nf) const { return spec && guard && spec->tm_supported(nf); }    // the front may write plane() tile-major
    int run(float2 *Z, uint32_t nf, void *out, hipStream_t s, bool tm)
    {
        int r;
        if (spec) {
            void *T = mixo ? (void *)d_B : out;
            if ((r = spec->run(Z, T, fm, nf, st, prm, fm_ref, fm ? rp.in() : nullptr, fm ? rp.out() : nullptr, s, tm))) return r;
            if (fm) rp.flip();
            return mixo ? launch_mix((const float *)T, (float *)out, C, fm ? nf : 2 * nf, s) : CSDR_OK;
        }
        if ((r = launch_agc(Z, C, nf, st, prm, s))) return r;
        if (fm) {
            float *F = mixo ? (float *)d_B : (float *)out;
            if ((r = launch_fm(Z, F, C, nf, fm_ref, rp.in(), rp.out(), s))) return r;
            rp.flip();
            if (mixo) return launch_mix(F, (float *)out, C, nf, s);
        } else if (mixo) return launch_mix((const float *)Z, (float *)out, C, 2 * nf, s);
        return CSDR_OK;
    }
    int stats(uint32_t *checked, uint32_t *redone) { return spec ? spec->stats(checked, redone) : 0; }
    uint32_t tile_major_calls() const { return spec ? spec->tm_calls : 0u; }
private:
    uint32_t C = 0; AgcParams prm; float fm_ref = 0.f;
    bool fm = false, mixo = false, in_place = false;
    const char *piece = "";
    AgcState *st = nullptr; PingPong<float2> rp;
    float2 *d_A = nullptr, *d_B = nullptr;    // Z, the plane between the front and the tail (guard readable elements on either side); the tail's output in front of --mix
    size_t guard = 0;
    std::optional<AgcTailPlan> spec;          // the time-parallel tail (kernels_agc_tail.hip); none: CSDR_FLAG_AGC_SEQUENTIAL
};

// DeAM = amDemodulator . agc: the chain runs as DeNo into input(), then the ampmodem peak detector (kernels_am.hip) [+ mix]
struct AmTail {
    int setup(DeviceBuffers &mem, uint32_t C_, uint32_t max_nf, bool mix_, std::string &path)
    {
        C = C_; mix = mix_;
        int r;
        if ((r = mem.alloc_n(&z, (size_t)C * max_nf))) return r;
        if (mix && (r = mem.alloc_n(&f, (size_t)C * max_nf))) return r;
        if ((r = q.alloc(mem, C))) return r;
        path += "+am";
        return CSDR_OK;
    }
    int reset(hipStream_t s) { return q.reset(s); }        // ampmodem_reset: q_hat = 0
    void *input() const { return z; }
    int run(uint32_t nf, void *out, uint32_t *n, hipStream_t s)      // *n: the elements in out
    {
        float *F = mix ? f : (float *)out;
        int r;
        if ((r = launch_am(z, F, C, nf, q.in(), q.out(), 0.01f, s))) return r;
        q.flip();
        if (mix && (r = launch_mix(F, (float *)out, C, nf, s))) return r;
        *n = mix ? nf : C * nf;
        return CSDR_OK;
    }
private:
    uint32_t C = 0; bool mix = false;
    float2 *z = nullptr; float *f = nullptr; PingPong<float> q;
};

// DeWBFM decim = firDecimator decim . iirDeemph . fmDemodulator 0.6 . agc: the chain runs as DeNBFM 0.6 into input(), then
// de-emphasis + decimator (kernels_wbfm.hip) [+ mix]
struct WbfmTail {
    int setup(DeviceBuffers &mem, const csdr_chain_cfg &cfg, uint32_t C_, uint32_t max_nf, bool mix_, std::string &path)
    {
        C = C_; mix = mix_;
        M = cfg.wbfm_decim ? cfg.wbfm_decim : 4u;
        const float fc = cfg.deemph_fc > 0.f ? cfg.deemph_fc : 0.025f;
        if (!(fc < 0.5f)) { set_error("chain: deemph_fc %g out of (0, 0.5)", fc); return CSDR_ERR_INVALID; }
        bq = design_butter2_lowpass(fc);
        const std::vector<float> taps = design_firdecim_kaiser(M, 10, 60.0f);
        hlen = (uint32_t)taps.size();
        const size_t rows = (size_t)C * max_nf;
        if (mem.alloc_n(&f, rows) || mem.alloc_n(&h, taps.size()) || hist.alloc(mem, (size_t)C * (hlen - 1)) || st.alloc(mem, C) ||
            (mix && mem.alloc_n(&o, rows))) {
            set_error("chain: WBFM tail allocation failed"); return CSDR_ERR_HIP;
        }
        CSDR_HIP(hipMemcpy(h, taps.data(), sizeof(float) * taps.size(), hipMemcpyHostToDevice));
        path += "+wbfm";
        return CSDR_OK;
    }
    int reset(hipStream_t s) { int r = st.reset(s); return r ? r : hist.reset(s); }
    void *input() const { return f; }
    uint32_t decim() const { return M; }                  // a call takes whole decimations
    int run(uint32_t nf, void *out, uint32_t *n, hipStream_t s)      // *n: the elements in out
    {
        const uint32_t no = nf / M;
        float *O = mix ? o : (float *)out;
        int r;
        if ((r = launch_biquad(f, f, C, nf, bq, st.in(), st.out(), s))) return r;
        if ((r = launch_firdecim(f, O, C, nf, M, h, hlen, hist.in(), hist.out(), s))) return r;
        st.flip(); hist.flip();
        if (mix && (r = launch_mix(O, (float *)out, C, no, s))) return r;
        *n = mix ? no : C * no;
        return CSDR_OK;
    }
private:
    uint32_t C = 0, M = 4, hlen = 0; bool mix = false; BiquadParams bq{};
    float *f = nullptr, *o = nullptr, *h = nullptr; PingPong<float> hist; PingPong<float2> st;
};

// CSDR_FLAG_DFT_BACKWARD: the chain as built (forward DFT) goes into input(); row k of the output = its row (M - k) mod M.  No state
struct RowReversal {
    int setup(DeviceBuffers &mem, uint32_t C_, uint32_t max_nf, uint32_t elem_, std::string &path)
    {
        C = C_; elem = elem_;
        int r = mem.alloc(&perm, (size_t)C * max_nf * elem); if (r) return r;
        path += "+dft-backward";
        return CSDR_OK;
    }
    void *input() const { return perm; }
    int run(uint32_t n, void *out, hipStream_t s) { return launch_rows_reversed(perm, out, C, (size_t)(n / C) * elem, s); }   // n elements in input()
private:
    uint32_t C = 0, elem = 8; void *perm = nullptr;
};
}  // namespace
}  // namespace csdr

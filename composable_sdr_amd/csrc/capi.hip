// C ABI of libcsdr_hip.so (see include/csdr.h): the route table and the chain handle (the plan of its route, the tails behind
// it, stream state and the per-chunk call sequence).  The handles of the single blocks are in capi_blocks.hip.  Product code: no CPU fallback,
// nothing from oracle/.
#include "../../include/csdr.h"
#include "capi_internal.h"
#include "fused.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

namespace csdr {
const char *last_error();
}
using namespace csdr;

struct csdr_chain {
    csdr_chain_cfg cfg;
    int device;
    uint32_t M, p, C, c0, max_nf; uint64_t max_nx;
    std::string path;
    // design
    std::vector<float> taps;
    uint32_t theta = 0, d_theta = 0;
    DcParams dc; AgcParams agc; float fm_ref = 0.f;
    // device memory (mem frees every buffer below with the handle)
    DeviceBuffers mem;
    uint32_t G = 1;                  // chan_stride: interleaved shard g = c0 of G
    bool dft_backward = false;       // CSDR_FLAG_DFT_BACKWARD: rows leave through d_perm and a row permutation k -> (M - k) mod M
    void *d_perm = nullptr;
    float2 *d_A = nullptr, *d_B = nullptr;     // AGC on: Z, the channel-major CF32 plane between the plan and the tail; the tail's output in front of --mix
    size_t a_guard = 0;              // fused chain with the AGC tail: d_A has this many readable elements in front of and behind the plane (tile-major route)
    AgcState *d_agc = nullptr;
    float2 *d_rp[2] = {nullptr, nullptr}; int rp_cur = 0;
    // host-API staging: CSDR_CHAIN_INFLIGHT slots (device in / out, page-locked host in / out), three streams
    struct HostSlot {
        float2 *d_in = nullptr; void *d_out = nullptr; void *h_in = nullptr, *h_out = nullptr;
        hipEvent_t e_in = nullptr, e_k = nullptr, e_out = nullptr;
        void *user_out = nullptr; uint32_t n_out = 0; size_t out_bytes = 0; bool staged_out = false;
    };
    HostSlot slot[CSDR_CHAIN_INFLIGHT];
    hipStream_t s_in = nullptr, s_k = nullptr, s_out = nullptr;
    uint32_t q_head = 0, q_count = 0;      // oldest pending slot, number of pending chunks
    ChainPlan *plan = nullptr;       // the route's plan (fused.h); null: CSDR_FLAG_TAIL_ONLY, the caller's rows are the front
    uint32_t n_cus = 256;            // compute units of the device (run counts of k_pfb1024 and of the plans: FusedConfig::cus)
    AgcTailPlan *agc_tail = nullptr; // AGC on: time-parallel verified tail (unless CSDR_FLAG_AGC_SEQUENTIAL)
    // DeAM: the chain runs as DeNo into d_amz, then the ampmodem peak detector (kernels_am.hip) [+ mix]
    bool tail_only = false;          // CSDR_FLAG_TAIL_ONLY: AGC [+ freqdem] [+ mix] on a channel-major CF32 plane
    bool am = false, am_mix = false;
    // DeWBFM: the chain runs as DeNBFM 0.6 into d_wbf, then de-emphasis + decimator (kernels_wbfm.hip) [+ mix]
    bool wbfm = false, wbfm_mix = false; uint32_t wb_decim = 4, wb_hlen = 0; BiquadParams wb_bq{};
    float *d_wbf = nullptr, *d_wbo = nullptr, *d_wbh = nullptr, *d_wbhist[2] = {nullptr, nullptr}; float2 *d_wbst[2] = {nullptr, nullptr}; int wb_cur = 0;
    float2 *d_amz = nullptr; float *d_amf = nullptr; float *d_amq[2] = {nullptr, nullptr}; int amq_cur = 0;
    KernelTimer timer;
    // pipelined device entry point (csdr_chain_submit_device): two handle-owned streams used alternately, so that consecutive
    // chunks' launches may overlap (the next launch's cold run starts fill the CUs the previous one has already left)
    hipStream_t s_pd[2] = {nullptr, nullptr};
    hipEvent_t e_pd_done[2] = {nullptr, nullptr}, e_pd_tail[3] = {nullptr, nullptr, nullptr}, e_serial = nullptr;
    bool pd_used[2] = {false, false}, pd_tail_rec = false, serial_pending = false, in_submit = false;
    uint32_t pd_count = 0, pd_indep_calls = 0;
    bool call_indep = false; hipEvent_t call_ev_tail = nullptr;     // handed to the plan by the call in progress
    // entry points share the handle's state: a call on a caller's stream is remembered so that the host-buffer entry point
    // (own stream s_k) can order itself behind it, and the other way round
    // (a handle-owned event recorded on the caller's stream behind the call's work: the caller may destroy the stream afterwards)
    hipEvent_t e_user = nullptr; bool user_stream_dirty = false;
    bool pd_last_indep = false;      // the previous csdr_chain_submit_device call ran as an independent launch
};

// a device buffer of the chain: n elements of T (at least one), freed with the handle
template <class T> static int chain_alloc(csdr_chain *h, T **p, size_t n) { return h->mem.alloc_n(p, n); }

extern "C" {

const char *csdr_last_error(void) { return csdr::last_error(); }
const char *csdr_version(void) { return "csdr-hip gfx950 0.1"; }

int csdr_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---------------------------------------------------------------------------
// fused chain
// ---------------------------------------------------------------------------
}  // extern "C"

// ---------------------------------------------------------------------------
// Route table: which plan and which kernels a chain configuration gets.  csdr_chain_create selects a row through
// route_select() and nothing else; csdr_route_table() prints the rows (README).  Per call the plan then picks
// between its run-sized and its chunk-sized kernel by the call's frame count (the thresholds are part of the row's text).
// ---------------------------------------------------------------------------
namespace {
constexpr uint32_t ST1 = 1u << 1, ST2 = 1u << 2, ST4 = 1u << 4, ST8 = 1u << 8, ST_ANY = ~0u;
struct RouteRow {
    uint32_t M;                 // channels the row is for; 0: any count
    uint32_t strides;           // bit g: chan_stride g accepted (bit 1: whole band or a contiguous shard)
    bool (*supported)(uint32_t M, uint32_t p);              // the plan takes M channels of p taps per branch
    int (*create)(const FusedConfig &cfg, ChainPlan **out);
    const char *path_prefix;    // csdr_chain_path of a fused row: prefix + the plan's kernel name [+interleaved-shard] [+agc] (ChainPlan::route)
    // shortest window of the plan: WU = 6 read-only warm-up tiles of 4096 samples (k_run256v2, k_run64v2, k_run1024v3, k_run1024v2),
    // H_WU = 7 frames of 4096 samples in front of a k_front4096 run
    double dc_window;
    const char *name, *run_sized, *other, *agc_tail;
};
const RouteRow ROUTES[] = {
    {256, ST1 | ST2 | ST4 | ST8, plan256_supported, plan256_create, "fused-256|", 6 * 4096.0, "fused-256",
     "k_run256v2<FM | CF32[, G]> (whole band: calls of >= 1024 whole tiles of 16 frames; interleaved shards G = 2, 4, 8: every whole tile)",
     "k_tile256<FM | CF32> (look-back tile kernel: chunk-sized calls, ragged ends, and contiguous channel shards at every size) [+ k_shard_gather]",
     "channelizer -> CF32 plane (tile-major for run-sized calls of whole tiles) -> k_agc_spec_tm | k_agc_spec -> k_agc_fix [-> k_mix]"},
    {64, ST1, plan64_supported, plan64_create, "fused-", 6 * 4096.0, "fused-k_run64",
     "k_run64v2 (CF32 output, whole band, nf % 64 == 0, >= 8 tiles of 64 frames per run)", "k_run64<FM | CF32> (FM output, shards, ragged calls)",
     "k_run64v2 -> CF32 plane (tile-major, run-sized calls) -> k_agc_spec_tm | k_run64<CF32> -> k_agc_spec; -> k_agc_fix [-> k_mix]"},
    {1024, ST1 | ST2 | ST4 | ST8, plan1024_supported, plan1024_create, "fused-", 6 * 4096.0, "fused-k_run1024",
     "k_run1024v3<FM | CF32> (whole band, calls of whole 4-frame tiles; a call that ends inside a 128-byte line stores the front part of it); "
     "k_shard1024<FM | CF32, G> (interleaved shards G = 4, 8: fold of the aliasing branches behind the FIR + a (1024 / G)-point DFT across the lanes; run-sized calls of whole tiles); "
     "k_run1024v2<FM, 2> (interleaved shards G = 2, FM output)",
     "k_run1024<FM | CF32> (ragged calls, contiguous shards, the other calls of interleaved shards) [+ k_pfb1024_fixup, k_shard_gather1024]", "k_run1024v3<CF32> -> CF32 plane (tile-major) -> k_agc_spec_tm | k_run1024<CF32> -> k_agc_spec; -> k_agc_fix [-> k_mix]"},
    {4096, ST1, plan4096_supported, plan4096_create, "fused-4096|", 7 * 4096.0, "fused-4096",
     "k_front4096 (DC blocker + pre-mix + FIR, branch-tiled: four sibling workgroups per frame, radix-4 split of the DFT on the registers) -> z (8 B / sample) "
     "-> k_back4096<CF32 | FM | FM,mix> (four 1024-point DFTs per frame, 16-frame blocks, whole 128-byte lines per row) [-> k_mix4096_finish]; whole band; "
     "DeNo --mix without the AGC keeps the any-M route's mix identity",
     "the same kernels (any call size; short calls use fewer runs)", "k_front4096 -> k_back4096<CF32> -> CF32 plane (tile-major: calls of whole 16-frame blocks, >= 4096 frames) -> k_agc_spec_tm | k_agc_spec -> k_agc_fix [-> k_mix]"},
    {0, ST_ANY, generic_supported, generic_create, nullptr, 0.0, "generic",
     "k_dc_tile -> k_pfb_fir (M = 1024, forced generic: k_pfb1024) -> k_fft_r16 | k_fft_pow2 | k_dft_direct [interleaved shard: k_fold + (M / G)-point DFT] "
     "-> k_transpose_fm | k_mix_frames | k_transpose;  DeNo --mix over all channels: k_dc_fold + k_mixid_finish (M % 4096 == 0) | k_dc_tile + k_branch0_fir "
     "(the sum of all bins of a frame is M x branch 0);  DeNo --mix of an interleaved shard (M % 4096 == 0, G = 2, 4, 8): k_dc_fold8 + k_mixid_shard_finish "
     "(the shard's channel sum is M / G x the phasor sum of the G surviving branches)",
     "the same kernels (any call size)", "... -> k_transpose -> k_agc_spec -> k_agc_fix [-> k_fm] [-> k_mix]"},
};
// dc: the handle's DC blocker, null without one.  Every fused plan truncates the DC state somewhere (warm-up windows, look-back tiles,
// dcfix); a handle whose alpha does not fit the plan's shortest window (dc_window_ok) takes the generic row.  The first row that takes
// the configuration: the last one (M = 0) takes them all.
const RouteRow *route_select(uint32_t M, uint32_t p, uint32_t G, uint32_t flags, const DcParams *dc)
{
    const bool fused = M > 1 && !(flags & CSDR_FLAG_FORCE_GENERIC) && !(G > 1 && diag_env("CSDR_SHARD_GENERIC"));
    const RouteRow *r = ROUTES;
    for (; r->M; r++) {
        if (!fused || r->M != M || !(G < 32 && (r->strides >> G) & 1u)) continue;
        if (dc && !dc_window_ok(*dc, r->dc_window)) continue;
        if (r->supported(M, p)) break;
    }
    return r;
}
std::string route_table_text()
{
    std::string t;
    char buf[256];
    for (const RouteRow &r : ROUTES) {
        std::string st;
        if (r.strides == ST_ANY) st = "any";
        else for (uint32_t g : {1u, 2u, 4u, 8u}) if ((r.strides >> g) & 1u) st += (st.empty() ? "" : ", ") + std::to_string(g);
        snprintf(buf, sizeof buf, "[%s] channels = %s, chan_stride in {%s}\n", r.name, r.M ? std::to_string(r.M).c_str() : "any", st.c_str());
        t += buf;
        t += std::string("    run-sized calls : ") + r.run_sized + "\n    other calls     : " + r.other + "\n    AGC on          : " + r.agc_tail + "\n";
    }
    t += "[tail-only] CSDR_FLAG_TAIL_ONLY: channel-major CF32 plane -> k_agc_spec -> k_agc_fix [-> k_mix] (hybrid multi-GPU partition)\n";
    return t;
}
}  // namespace

extern "C" {

const char *csdr_route_table(void)
{
    static const std::string text = route_table_text();
    return text.c_str();
}

void csdr_chain_cfg_default(csdr_chain_cfg *cfg, uint32_t channels)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = sizeof(*cfg);
    cfg->channels = channels ? channels : 1;
    cfg->dc_block = 1;
    cfg->dc_alpha = 0.0005f;
    cfg->agc_threshold_db = 0.0f;
    cfg->demod = CSDR_DEMOD_NONE;
    cfg->kf = 0.3f;
    cfg->device = -1;
    cfg->max_frames = 4096;
    cfg->pfb_m = 7;
    cfg->pfb_as = 80.0f;
    cfg->wbfm_decim = 4;
    cfg->deemph_fc = 0.025f;
}

static int chain_init_state(csdr_chain *h, hipStream_t s)
{
    h->theta = 0; h->rp_cur = 0;
    if (h->d_agc) { int r = launch_agc_init(h->d_agc, h->C, s); if (r) return r; }
    if (h->agc_tail) agc_tail_reset(h->agc_tail);
    if (h->d_rp[0]) {
        CSDR_HIP(hipMemsetAsync(h->d_rp[0], 0, sizeof(float2) * h->C, s));
        CSDR_HIP(hipMemsetAsync(h->d_rp[1], 0, sizeof(float2) * h->C, s));
    }
    if (h->d_wbst[0]) {
        h->wb_cur = 0;
        for (int i = 0; i < 2; i++) {
            CSDR_HIP(hipMemsetAsync(h->d_wbst[i], 0, sizeof(float2) * h->C, s));
            CSDR_HIP(hipMemsetAsync(h->d_wbhist[i], 0, sizeof(float) * (size_t)h->C * (h->wb_hlen - 1), s));
        }
    }
    if (h->d_amq[0]) {
        h->amq_cur = 0;
        CSDR_HIP(hipMemsetAsync(h->d_amq[0], 0, sizeof(float) * h->C, s));     // ampmodem_reset: q_hat = 0
        CSDR_HIP(hipMemsetAsync(h->d_amq[1], 0, sizeof(float) * h->C, s));
    }
    return h->plan ? h->plan->reset(s) : 0;
}

int csdr_chain_create(const csdr_chain_cfg *cfg_in, csdr_chain **out)
{
    if (!cfg_in || !out) { set_error("chain: null argument"); return CSDR_ERR_INVALID; }
    if (cfg_in->struct_size != sizeof(csdr_chain_cfg)) { set_error("chain: cfg.struct_size %u != %zu", cfg_in->struct_size, sizeof(csdr_chain_cfg)); return CSDR_ERR_INVALID; }
    if (cfg_in->demod > CSDR_DEMOD_WBFM) { set_error("chain: unknown demod %u", cfg_in->demod); return CSDR_ERR_INVALID; }
    // DeAM = amDemodulator . agc (SoapySDR.hs:265-272): everything up to the per-channel CF32 samples is the DeNo
    // chain; the peak detector and the mix follow as a tail (see csdr_chain_process_device)
    csdr_chain_cfg eff = *cfg_in;
    const bool am = cfg_in->demod == CSDR_DEMOD_AM, am_mix = am && cfg_in->mix != 0 && cfg_in->channels > 1;
    if (am) { eff.demod = CSDR_DEMOD_NONE; eff.mix = 0; }
    // DeWBFM decim = firDecimator decim . iirDeemph . fmDemodulator 0.6 . agc (SoapySDR.hs:252-259, Liquid.chs:653-656)
    const bool wbfm = cfg_in->demod == CSDR_DEMOD_WBFM, wbfm_mix = wbfm && cfg_in->mix != 0 && cfg_in->channels > 1;
    if (wbfm) { eff.demod = CSDR_DEMOD_FM; eff.kf = 0.6f; eff.mix = 0; }
    const csdr_chain_cfg *cfg = &eff;
    if (cfg->channels < 1 || cfg->channels > (1u << 16)) { set_error("chain: channels %u out of range", cfg->channels); return CSDR_ERR_INVALID; }
    if (cfg_in->flags & CSDR_FLAG_TAIL_ONLY) {
        // the per-channel tail alone (hybrid multi-GPU partition): rows in, rows out; state = AGC {g, y2', mode, timer} + freqdem r' per row
        if (cfg_in->agc_threshold_db == 0.0f || am || wbfm) { set_error("chain: CSDR_FLAG_TAIL_ONLY needs the AGC on (-a != 0) and demod none / FM (without the AGC a time stripe needs no tail shard)"); return CSDR_ERR_INVALID; }
        if (cfg->demod == CSDR_DEMOD_FM && !(cfg->kf > 0.f)) { set_error("chain: FM needs kf > 0"); return CSDR_ERR_INVALID; }
        int dev; int r = check_device(cfg->device, &dev); if (r) return r;
        DevGuard guard(dev);
        if (!guard.ok) { set_error("chain: cannot select device %d", dev); return CSDR_ERR_HIP; }
        csdr_chain *h = new (std::nothrow) csdr_chain();
        if (!h) return CSDR_ERR_NOMEM;
        h->cfg = *cfg; h->cfg.chan_first = 0; h->cfg.chan_count = 0; h->cfg.chan_stride = 0; h->cfg.dc_block = 0;
        h->device = dev; h->tail_only = true;
        h->M = cfg->channels; h->C = cfg->channels; h->c0 = 0; h->G = 1; h->p = 0;
        h->max_nf = cfg->max_frames ? cfg->max_frames : 4096;
        h->max_nx = (uint64_t)h->max_nf * h->M;
        if (h->max_nx > 0xffffffffull) { set_error("chain: max_frames*channels exceeds 2^32-1 samples"); delete h; return CSDR_ERR_INVALID; }
        h->agc = make_agc(cfg->agc_threshold_db);
        if (cfg->demod == CSDR_DEMOD_FM) h->fm_ref = fm_ref_of(cfg->kf);
        auto failt = [&](int code) { csdr_chain_destroy(h); return code; };
        if ((r = chain_alloc(h, &h->d_agc, h->C))) return failt(r);
        if (cfg->demod == CSDR_DEMOD_FM && ((r = chain_alloc(h, &h->d_rp[0], h->C)) || (r = chain_alloc(h, &h->d_rp[1], h->C)))) return failt(r);
        if (cfg->mix && h->C > 1 && (r = chain_alloc(h, &h->d_B, (size_t)h->C * h->max_nf))) return failt(r);
        if (!(cfg->flags & CSDR_FLAG_AGC_SEQUENTIAL)) { if ((r = agc_tail_create(h->C, h->max_nf, &h->agc_tail))) return failt(r); }
        else if ((r = chain_alloc(h, &h->d_A, (size_t)h->C * h->max_nf))) return failt(r);        // the one-lane-per-channel kernel works in place
        h->path = std::string("tail-only+agc") + (h->agc_tail ? "-spec" : "");
        if ((r = chain_init_state(h, nullptr))) return failt(r);
        CSDR_HIP_CLEAN(hipDeviceSynchronize(), csdr_chain_destroy(h));
        if (!(cfg->flags & CSDR_FLAG_QUIET)) {
            printf("csdr chain [%s] on HIP device %d: %u channel rows, agc=%g dB demod=%s kf=%g mix=%u\n", h->path.c_str(), dev, h->C,
                   cfg->agc_threshold_db, cfg->demod == CSDR_DEMOD_FM ? "FM" : "none", cfg->kf, cfg->mix);
            fflush(stdout);
        }
        *out = h;
        return CSDR_OK;
    }
    if (cfg->demod == CSDR_DEMOD_FM && !(cfg->kf > 0.f)) { set_error("chain: FM needs kf > 0"); return CSDR_ERR_INVALID; }
    if (cfg->dc_block && !(cfg->dc_alpha > 0.f && cfg->dc_alpha < 1.f)) { set_error("chain: dc_alpha out of (0,1)"); return CSDR_ERR_INVALID; }
    if (cfg->pfb_m > 32u) { set_error("chain: pfb_m %u out of 1..32 (0 = 7)", cfg->pfb_m); return CSDR_ERR_INVALID; }
    const uint32_t M = cfg->channels;
    uint32_t c0 = cfg->chan_first, C = cfg->chan_count ? cfg->chan_count : M - c0;
    const uint32_t G = cfg->chan_stride > 1 ? cfg->chan_stride : 1;
    if (G > 1) {
        if (M % G || c0 >= G || (cfg->chan_count && cfg->chan_count != M / G)) {
            set_error("chain: interleaved shard %u of %u needs chan_stride | channels (%u), chan_first < chan_stride, chan_count 0 or channels/chan_stride", c0, G, M);
            return CSDR_ERR_INVALID;
        }
        C = M / G;
    } else if (c0 >= M || C == 0 || c0 + C > M) { set_error("chain: channel shard [%u,+%u) outside 0..%u", c0, C, M); return CSDR_ERR_INVALID; }
    int dev; int r = check_device(cfg->device, &dev); if (r) return r;
    DevGuard guard(dev);
    if (!guard.ok) { set_error("chain: cannot select device %d", dev); return CSDR_ERR_HIP; }

    csdr_chain *h = new (std::nothrow) csdr_chain();
    if (!h) return CSDR_ERR_NOMEM;
    h->cfg = *cfg; h->device = dev; h->M = M; h->C = C; h->c0 = c0; h->G = G;
    { int cus = 256; (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev); h->n_cus = (uint32_t)cus; }
    const uint32_t m = cfg->pfb_m ? cfg->pfb_m : 7;
    const float As = cfg->pfb_as > 0.f ? cfg->pfb_as : 80.0f;
    h->p = 2 * m;
    h->max_nf = cfg->max_frames ? cfg->max_frames : 4096;
    h->max_nx = (uint64_t)h->max_nf * M;
    if (h->max_nx > 0xffffffffull) { set_error("chain: max_frames*channels exceeds 2^32-1 samples"); delete h; return CSDR_ERR_INVALID; }
    h->timer.enabled = (cfg->flags & (CSDR_FLAG_TIME_KERNELS | CSDR_FLAG_TIME_REGION)) != 0;
    h->timer.region = (cfg->flags & CSDR_FLAG_TIME_REGION) != 0;
    if (cfg->dc_block) h->dc = make_dc(cfg->dc_alpha);
    if (cfg->agc_threshold_db != 0.0f) h->agc = make_agc(cfg->agc_threshold_db);
    if (cfg->demod == CSDR_DEMOD_FM) h->fm_ref = fm_ref_of(cfg->kf);

    auto fail = [&](int code) { csdr_chain_destroy(h); return code; };
    if (M > 1) {
        h->taps = design_pfb_taps(M, m, As);
        h->d_theta = nco_freq_word(pfb_premix_freq(M));
    }
    if (cfg->agc_threshold_db != 0.0f && (r = chain_alloc(h, &h->d_agc, C))) return fail(r);
    // (without the AGC the plan does the freqdem and keeps its history)
    if (cfg->agc_threshold_db != 0.0f && cfg->demod == CSDR_DEMOD_FM && ((r = chain_alloc(h, &h->d_rp[0], C)) || (r = chain_alloc(h, &h->d_rp[1], C)))) return fail(r);

    // Path selection.  With the AGC on, the plan stops at the channel-major CF32 samples and the per-channel AGC tail (time-parallel, or
    // with CSDR_FLAG_AGC_SEQUENTIAL one lane per channel) + freqdem + mix follow.
    // interleaved shards: the fused M = 256 and 1024 chains take strides 2, 4, 8; every other shape the any-M route with a pruned DFT
    const DcParams *dcp = cfg->dc_block ? &h->dc : nullptr;
    const RouteRow *route = route_select(M, h->p, G, cfg->flags, dcp);     // the one place a configuration is mapped to a plan (table above)
    if (route->M == 4096 && (C != M || (cfg->mix && cfg->demod == CSDR_DEMOD_NONE && cfg->agc_threshold_db == 0.0f && !am)))
        route = route_select(M, h->p, G, cfg->flags | CSDR_FLAG_FORCE_GENERIC, dcp);   // contiguous shards; DeNo --mix over all channels (= M x branch 0: nothing beats not computing
                                                                                   // the bank; CSDR_FLAG_NO_MIX_IDENTITY's full bank + DFT + sum stays on the any-M kernels too)
    const bool agc_on = cfg->agc_threshold_db != 0.0f;
    FusedConfig fc{};
    fc.M = M; fc.p = h->p; fc.C = C; fc.c0 = c0; fc.max_nf = h->max_nf; fc.G = G;
    fc.dc_block = cfg->dc_block != 0; fc.dc = h->dc;
    fc.fm = cfg->demod == CSDR_DEMOD_FM && !agc_on; fc.fm_ref = h->fm_ref;
    fc.mix = cfg->mix != 0 && !agc_on; fc.taps = h->taps.data(); fc.d_theta = h->d_theta; fc.cus = h->n_cus;
    fc.no_mix_identity = (cfg->flags & CSDR_FLAG_NO_MIX_IDENTITY) != 0;
    if ((r = route->create(fc, &h->plan))) return fail(r);
    const std::string front = h->plan->route(route->path_prefix, agc_on);
    h->path = front;
    if (agc_on) {
        // d_A: channel-major CF32 from the plan; d_B: per-channel tail output in front of --mix
        // (the fused plans may write d_A tile-major for k_agc_spec_tm, which reads up to a segment in front of / behind the plane)
        // The guards (2 x 64 KiB per channel: 128 MiB at 1024 channels) exist only where a call can take that route: a fused plan (the any-M
        // plan never writes tile-major), a time-parallel tail (not CSDR_FLAG_AGC_SEQUENTIAL), a channel count k_agc_spec_tm takes, calls
        // of >= 4 W = 4096 frames
        const bool tm_possible = route->M && !(cfg->flags & CSDR_FLAG_AGC_SEQUENTIAL) && h->max_nf >= 4096u &&
                                 (C % 64u == 0 || (C < 64u && 64u % C == 0));
        h->a_guard = tm_possible ? agc_tail_tm_guard(C) : 0;
        if ((r = chain_alloc(h, &h->d_A, (size_t)C * h->max_nf + 2 * h->a_guard))) return fail(r);
        if (h->a_guard) {
            // only the guards need defined contents (the warm-ups of the first and last segments read them, masked by position)
            CSDR_HIP_CLEAN(hipMemset(h->d_A, 0, sizeof(float2) * h->a_guard), csdr_chain_destroy(h));
            CSDR_HIP_CLEAN(hipMemset(h->d_A + h->a_guard + (size_t)C * h->max_nf, 0, sizeof(float2) * h->a_guard), csdr_chain_destroy(h));
        }
        if (cfg->mix && (r = chain_alloc(h, &h->d_B, (size_t)C * h->max_nf))) return fail(r);
    }
    if ((cfg_in->flags & CSDR_FLAG_DFT_BACKWARD) && M > 1 && !(cfg_in->mix != 0)) {
        if (C != M || G > 1) { set_error("chain: CSDR_FLAG_DFT_BACKWARD is built for whole-band handles (no channel shard)"); return fail(CSDR_ERR_INVALID); }
        h->dft_backward = true;
        if ((r = h->mem.alloc(&h->d_perm, (size_t)C * h->max_nf * ((cfg_in->demod == CSDR_DEMOD_NONE) ? 8u : 4u)))) return fail(r);
        h->path += "+dft-backward";
    }
    if (am) {
        h->am = true; h->am_mix = am_mix;
        if ((r = chain_alloc(h, &h->d_amz, (size_t)C * h->max_nf))) return fail(r);
        if (am_mix && (r = chain_alloc(h, &h->d_amf, (size_t)C * h->max_nf))) return fail(r);
        if ((r = chain_alloc(h, &h->d_amq[0], C)) || (r = chain_alloc(h, &h->d_amq[1], C))) return fail(r);
        h->path += "+am";
    }
    if (wbfm) {
        h->wbfm = true; h->wbfm_mix = wbfm_mix;
        h->wb_decim = cfg_in->wbfm_decim ? cfg_in->wbfm_decim : 4u;
        const float fc = cfg_in->deemph_fc > 0.f ? cfg_in->deemph_fc : 0.025f;
        if (!(fc < 0.5f)) { set_error("chain: deemph_fc %g out of (0, 0.5)", fc); return fail(CSDR_ERR_INVALID); }
        h->wb_bq = design_butter2_lowpass(fc);
        const std::vector<float> taps = design_firdecim_kaiser(h->wb_decim, 10, 60.0f);
        h->wb_hlen = (uint32_t)taps.size();
        const size_t rows = (size_t)C * h->max_nf, hist = (size_t)C * (h->wb_hlen - 1);
        if (chain_alloc(h, &h->d_wbf, rows) || chain_alloc(h, &h->d_wbh, taps.size()) || chain_alloc(h, &h->d_wbhist[0], hist) || chain_alloc(h, &h->d_wbhist[1], hist) ||
            chain_alloc(h, &h->d_wbst[0], C) || chain_alloc(h, &h->d_wbst[1], C) || (wbfm_mix && chain_alloc(h, &h->d_wbo, rows))) {
            set_error("chain: WBFM tail allocation failed"); return fail(CSDR_ERR_HIP);
        }
        CSDR_HIP_CLEAN(hipMemcpy(h->d_wbh, taps.data(), sizeof(float) * taps.size(), hipMemcpyHostToDevice), csdr_chain_destroy(h));
        h->path += "+wbfm";
    }
    if (h->d_agc && !(cfg->flags & CSDR_FLAG_AGC_SEQUENTIAL)) {
        if ((r = agc_tail_create(C, h->max_nf, &h->agc_tail))) return fail(r);
        h->path += route->M ? "-spec" : "+agc-spec";      // (a fused row's text already says +agc)
    }
    if ((r = chain_init_state(h, nullptr))) return fail(r);
    CSDR_HIP_CLEAN(hipDeviceSynchronize(), csdr_chain_destroy(h));

    if (!(cfg->flags & CSDR_FLAG_QUIET)) {
        // what the reference prints at create (Liquid.chs:577-579, 814-820, 714-716, 319-321)
        printf("csdr chain [%s] on HIP device %d: channels=%u (shard %u..%u) taps=%u (m=%u, As=%.1f) "
               "nco.d_theta=0x%08x dc_block=%u(alpha=%g) agc=%g dB demod=%s kf=%g mix=%u\n",
               h->path.c_str(), dev, M, c0, c0 + C - 1, M > 1 ? M * h->p : 0, m, As, h->d_theta, cfg->dc_block,
               cfg->dc_alpha, cfg->agc_threshold_db, am ? "AM" : (wbfm ? "WBFM" : (cfg->demod == CSDR_DEMOD_FM ? "FM" : "none")), cfg->kf, cfg_in->mix);
        // per-channel outputs / AGC / demod tails beyond the fused kernels' channel counts run stage by stage through HBM
        if (!route->M && M > 1024 && front != "generic+mix-identity")
            printf("csdr chain: note: %u channels with per-channel output run on the any-M route (DC blocker, FIR, DFT and tail as separate kernels, "
                   "~0.09 of the HBM roofline on MI355X); fused kernels exist for 64, 256 and 1024 channels, and for DeNo --mix over all channels of any count\n", M);
        fflush(stdout);
    }
    *out = h;
    return CSDR_OK;
}

uint32_t csdr_chain_out_elem_size(const csdr_chain *h) { return h && (h->cfg.demod == CSDR_DEMOD_FM || h->am || h->wbfm) ? 4u : 8u; }

// Z[C][nf] (channel-major CF32) -> AGC + squelch [+ freqdem] [+ mix] -> d_out: the time-parallel tail (tm: Z tile-major), or with
// CSDR_FLAG_AGC_SEQUENTIAL one lane per channel in place on Z
static int chain_tail(csdr_chain *h, float2 *Z, uint32_t nf, void *d_out, hipStream_t s, bool tm)
{
    const bool fm = h->cfg.demod == CSDR_DEMOD_FM, mixo = h->cfg.mix && h->M > 1;
    int r;
    if (h->agc_tail) {
        void *T = mixo ? (void *)h->d_B : d_out;
        if ((r = agc_tail_process(h->agc_tail, Z, T, fm, nf, h->d_agc, h->agc, h->fm_ref,
                                  fm ? h->d_rp[h->rp_cur] : nullptr, fm ? h->d_rp[h->rp_cur ^ 1] : nullptr, s, tm))) return r;
        if (fm) h->rp_cur ^= 1;
        if (mixo) return launch_mix((const float *)T, (float *)d_out, h->C, fm ? nf : 2 * nf, s);
        return 0;
    }
    if ((r = launch_agc(Z, h->C, nf, h->d_agc, h->agc, s))) return r;
    if (fm) {
        float *F = mixo ? (float *)h->d_B : (float *)d_out;
        if ((r = launch_fm(Z, F, h->C, nf, h->fm_ref, h->d_rp[h->rp_cur], h->d_rp[h->rp_cur ^ 1], s))) return r;
        h->rp_cur ^= 1;
        if (mixo) return launch_mix(F, (float *)d_out, h->C, nf, s);
    } else if (mixo) return launch_mix((const float *)Z, (float *)d_out, h->C, 2 * nf, s);
    return 0;
}

// The argument checks of every entry point that takes a chunk (texts and codes are part of the C ABI), then the handle's device
static int chain_check_chunk(const csdr_chain *h, const void *in, uint32_t n_in, const void *out, DevGuard &guard)
{
    if (n_in && (!in || !out)) { set_error("chain: null buffer"); return CSDR_ERR_INVALID; }
    if (n_in % h->M) { set_error("chain: n_in=%u is not a multiple of channels=%u (the reference misbehaves here; Liquid.chs:832-862)", n_in, h->M); return CSDR_ERR_SIZE; }
    if (n_in > h->max_nx) { set_error("chain: n_in=%u exceeds max_frames*channels=%llu", n_in, (unsigned long long)h->max_nx); return CSDR_ERR_SIZE; }
    guard.select(h->device);
    if (!guard.ok) { set_error("chain: cannot select device %d", h->device); return CSDR_ERR_HIP; }
    return CSDR_OK;
}

// One call on stream: the plan (tail-only: the caller's rows), the AGC tail, the AM or the WBFM tail, the backward handle's row
// reversal.  Every stage writes the next stage's input, the last one d_out.
static int chain_call(csdr_chain *h, const void *d_in, uint32_t n_in, void *d_out, uint32_t *n_out, void *stream)
{
    // 1. checks (texts, codes and their order are part of the C ABI)
    if (!h) { set_error("chain: null handle"); return CSDR_ERR_INVALID; }
    const bool backward = h->dft_backward && n_in && d_out;     // (with nothing to do or nowhere to put it a backward handle answers as a forward one)
    if (n_out && !backward) *n_out = 0;                         // (a call a backward handle refuses has always left *n_out alone)
    if (n_in == 0) return CSDR_OK;
    if (!d_out) { set_error("chain: null buffer"); return CSDR_ERR_INVALID; }
    if (h->wbfm && n_in % h->M == 0 && (n_in / h->M) % h->wb_decim) {
        set_error("chain: %u frames per call are not a multiple of the WBFM decimation %u (firDecim's `div`, Liquid.chs:495-497)", n_in / h->M, h->wb_decim);
        return CSDR_ERR_SIZE;
    }
    DevGuard guard;
    int r;
    if ((r = chain_check_chunk(h, d_in, n_in, d_out, guard))) return r;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t nf = n_in / h->M, C = h->C;
    const bool agc_on = h->d_agc != nullptr, fm = h->cfg.demod == CSDR_DEMOD_FM, mixo = h->cfg.mix && h->M > 1;
    void *const last = backward ? h->d_perm : d_out;                                      // output of stage 4
    void *const chain_out = h->wbfm ? (void *)h->d_wbf : h->am ? (void *)h->d_amz : last;   // output of stages 2 + 3
    uint32_t n = mixo ? nf : C * nf;                                                      // elements in it

    // 2. front: the route's plan writes Z: chain_out, or with the AGC on the plane its tail reads (chain_out itself where the sequential
    // AGC is the last step and works in place).  Tail-only: Z = the caller's rows (the sequential AGC works in place on a copy)
    float2 *Z = (agc_on && (fm || mixo || h->agc_tail)) ? h->d_A + h->a_guard : (float2 *)chain_out;
    bool tm = false;
    if (h->plan) {
        FusedCall fcall{};
        // time-parallel AGC tail behind a fused plan, run-sized calls of whole tiles: the plane between the two kernels is tile-major
        tm = h->agc_tail && h->a_guard && agc_tail_tm_supported(h->agc_tail, nf) && h->plan->tile_major_ok(nf);
        fcall.tile_major = tm;
        fcall.d_in = (const float2 *)d_in; fcall.d_out = Z; fcall.nf = nf; fcall.theta0 = h->theta;
        fcall.indep = h->call_indep; fcall.ev_tail = h->call_ev_tail;
        if ((r = h->plan->process(fcall, s, &h->timer))) return r;
        h->theta += n_in * h->d_theta;     // the NCO phase behind the call
    } else if (h->agc_tail) Z = (float2 *)d_in;
    else { Z = h->d_A; CSDR_HIP(hipMemcpyAsync(Z, d_in, sizeof(float2) * (size_t)n_in, hipMemcpyDeviceToDevice, s)); }

    // 3. AGC + squelch [+ freqdem] [+ mix]
    if (agc_on && (r = chain_tail(h, Z, nf, chain_out, s, tm))) return r;
    if (!h->plan && !h->agc_tail && !fm && !mixo) CSDR_HIP(hipMemcpyAsync(chain_out, Z, sizeof(float2) * (size_t)n_in, hipMemcpyDeviceToDevice, s));

    // 4. DeWBFM: the chain ran as DeNBFM 0.6; de-emphasis + decimator [+ mix].  DeAM: it ran as DeNo; the ampmodem peak detector [+ mix]
    if (h->wbfm) {
        const uint32_t no = nf / h->wb_decim;
        if ((r = launch_biquad(h->d_wbf, h->d_wbf, C, nf, h->wb_bq, h->d_wbst[h->wb_cur], h->d_wbst[h->wb_cur ^ 1], s))) return r;
        float *O = h->wbfm_mix ? h->d_wbo : (float *)last;
        if ((r = launch_firdecim(h->d_wbf, O, C, nf, h->wb_decim, h->d_wbh, h->wb_hlen, h->d_wbhist[h->wb_cur], h->d_wbhist[h->wb_cur ^ 1], s))) return r;
        h->wb_cur ^= 1;
        if (h->wbfm_mix && (r = launch_mix(O, (float *)last, C, no, s))) return r;
        n = h->wbfm_mix ? no : C * no;
    } else if (h->am) {
        float *F = h->am_mix ? h->d_amf : (float *)last;
        if ((r = launch_am(h->d_amz, F, C, nf, h->d_amq[h->amq_cur], h->d_amq[h->amq_cur ^ 1], 0.01f, s))) return r;
        h->amq_cur ^= 1;
        if (h->am_mix && (r = launch_mix(F, (float *)last, C, nf, s))) return r;
        n = h->am_mix ? nf : C * nf;
    }
    if (n_out) *n_out = n;

    // 5. CSDR_FLAG_DFT_BACKWARD: the chain as built (forward DFT) went into d_perm; row k of the output = its row (M - k) mod M
    if (backward) return launch_rows_reversed(h->d_perm, d_out, C, (size_t)(n / C) * csdr_chain_out_elem_size(h), s);
    return CSDR_OK;
}

// A call on a caller's stream is remembered by an event behind its work, so that the host-buffer entry point (own stream s_k) can
// order itself behind it without keeping the caller's stream handle
static int chain_mark_user_stream(csdr_chain *h, hipStream_t stream)
{
    // only a handle that has used its host-buffer entry points has anything to order against (no event record per call on
    // the device-only hot path, and none inside a caller's stream capture); the first host-buffer call synchronises the device once
    if (!h->s_k) return CSDR_OK;
    if (!h->e_user) CSDR_HIP(hipEventCreateWithFlags(&h->e_user, hipEventDisableTiming));
    CSDR_HIP(hipEventRecord(h->e_user, stream));
    h->user_stream_dirty = true;
    return CSDR_OK;
}

int csdr_chain_process_device(csdr_chain *h, const void *d_in, uint32_t n_in, void *d_out, uint32_t *n_out, void *stream)
{
    if (!h || h->in_submit) return chain_call(h, d_in, n_in, d_out, n_out, stream);
    const bool own = h->s_k && (hipStream_t)stream == h->s_k;       // called by csdr_chain_submit / csdr_chain_process on the handle's stream
    DevGuard guard(h->device);
    if (!own && h->s_k && h->q_count) CSDR_HIP(hipStreamSynchronize(h->s_k));   // host-buffer chunks still in flight come first
    if (h->s_pd[0]) {
        // the handle has pipelined chunks (csdr_chain_submit_device): this call follows them, and a later submit follows this call
        for (int i = 0; i < 2; i++) if (h->pd_used[i]) CSDR_HIP(hipStreamWaitEvent((hipStream_t)stream, h->e_pd_done[i], 0));
    }
    int r = chain_call(h, d_in, n_in, d_out, n_out, stream);
    if (r) return r;
    if (h->s_pd[0]) {
        CSDR_HIP(hipEventRecord(h->e_serial, (hipStream_t)stream));
        h->serial_pending = true;
    }
    return own ? CSDR_OK : chain_mark_user_stream(h, (hipStream_t)stream);
}

// Device-side spin-wait time-outs (k_tile256 look-back / hand-off, k_dc_tile look-back) set a sticky status word and the
// kernel carries on with garbage carries: report it as an error once, then clear it.  Synchronises the device.
static int chain_device_status(csdr_chain *h)
{
    unsigned st = 0;
    int r;
    if (h->plan && (r = h->plan->status(&st))) return r;
    if (st) {
        set_error("chain: an inter-workgroup wait timed out on the device (plan status 0x%x): the output of the affected calls is invalid", st);
        return CSDR_ERR_HIP;
    }
    return CSDR_OK;
}

int csdr_chain_status(csdr_chain *h)
{
    if (!h) { set_error("chain: null handle"); return CSDR_ERR_INVALID; }
    DevGuard guard(h->device);
    return chain_device_status(h);
}

int csdr_chain_submit_device(csdr_chain *h, const void *d_in, uint32_t n_in, void *d_out, uint32_t *n_out, void *ready_event)
{
    if (!h) { set_error("chain: null handle"); return CSDR_ERR_INVALID; }
    if (n_out) *n_out = 0;
    if (n_in == 0) return CSDR_OK;
    DevGuard guard;
    if (int r = chain_check_chunk(h, d_in, n_in, d_out, guard)) return r;
    if (!h->s_pd[0]) {
        CSDR_HIP(hipDeviceSynchronize());               // whatever the handle has queued on caller streams so far
        // created into locals and published together: a partial failure leaves the handle as it was
        hipStream_t st[2] = {nullptr, nullptr}; hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        bool ok = true;
        for (int i = 0; i < 2 && ok; i++) ok = hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking) == hipSuccess;
        for (int i = 0; i < 6 && ok; i++) ok = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            for (hipStream_t q : st) if (q) (void)hipStreamDestroy(q);
            for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
            (void)hipGetLastError();
            set_error("chain: cannot create the streams / events of the pipelined entry point");
            return CSDR_ERR_HIP;
        }
        for (int i = 0; i < 2; i++) { h->s_pd[i] = st[i]; h->e_pd_done[i] = ev[i]; }
        for (int i = 0; i < 3; i++) h->e_pd_tail[i] = ev[2 + i];
        h->e_serial = ev[5];
        if (h->plan) h->plan->keep_tail();
    }
    if (h->s_k && h->q_count) CSDR_HIP(hipStreamSynchronize(h->s_k));       // host-buffer chunks still in flight come first
    const uint32_t nf = n_in / h->M, k = h->pd_count;
    const int si = (int)(k & 1);
    hipStream_t s = h->s_pd[si];
    // An independent launch (fused M = 256 chain without AGC / AM / WBFM tails, run-kernel-sized whole-tile chunk, previous
    // chunk's tail on file) reads nothing an earlier launch writes: it only waits for the input and for the copy of the
    // previous chunk's tail.  Every other call is ordered behind everything the handle has in flight.
    const bool overlap = h->plan && !h->d_agc && !h->am && !h->wbfm && h->plan->can_overlap(nf);
    if (ready_event) CSDR_HIP(hipStreamWaitEvent(s, (hipEvent_t)ready_event, 0));
    if (h->serial_pending) { CSDR_HIP(hipStreamWaitEvent(s, h->e_serial, 0)); h->serial_pending = false; }
    if (overlap) {
        if (h->pd_tail_rec) CSDR_HIP(hipStreamWaitEvent(s, h->e_pd_tail[(k + 2) % 3], 0));       // recorded by call k - 1
        // a call k - 1 that was NOT independent reads the plan's ping-pong state (run 0) that this launch's last run overwrites:
        // then this launch follows all of it, not only its tail copy
        if (!h->pd_last_indep && h->pd_used[si ^ 1]) CSDR_HIP(hipStreamWaitEvent(s, h->e_pd_done[si ^ 1], 0));
    } else if (h->pd_used[si ^ 1]) CSDR_HIP(hipStreamWaitEvent(s, h->e_pd_done[si ^ 1], 0));
    h->call_indep = overlap; h->call_ev_tail = h->e_pd_tail[k % 3]; h->in_submit = true;
    const int r = csdr_chain_process_device(h, d_in, n_in, d_out, n_out, s);
    h->call_indep = false; h->call_ev_tail = nullptr; h->in_submit = false;
    if (r) return r;
    h->pd_tail_rec = h->plan && h->plan->tail_recorded();
    if (overlap) h->pd_indep_calls++;
    h->pd_last_indep = overlap;
    CSDR_HIP(hipEventRecord(h->e_pd_done[si], s));
    h->pd_used[si] = true; h->pd_count = k + 1;
    return CSDR_OK;
}

uint32_t csdr_chain_debug_independent_launches(const csdr_chain *h) { return h ? h->pd_indep_calls : 0u; }

int csdr_chain_wait_device(csdr_chain *h, void *stream)
{
    if (!h) { set_error("chain: null handle"); return CSDR_ERR_INVALID; }
    DevGuard guard(h->device);
    for (int i = 0; i < 2; i++) {
        if (!h->pd_used[i]) continue;
        if (stream) CSDR_HIP(hipStreamWaitEvent((hipStream_t)stream, h->e_pd_done[i], 0));
        else CSDR_HIP(hipEventSynchronize(h->e_pd_done[i]));
    }
    return CSDR_OK;
}

void *csdr_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void csdr_host_free(void *p) { if (p) (void)hipHostFree(p); }

static bool is_pinned(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

static int chain_host_init(csdr_chain *h)
{
    if (h->s_k) return CSDR_OK;
    CSDR_HIP(hipDeviceSynchronize());                   // whatever csdr_chain_process_device calls have queued on caller streams so far
    CSDR_HIP(hipStreamCreateWithFlags(&h->s_in, hipStreamNonBlocking));
    CSDR_HIP(hipStreamCreateWithFlags(&h->s_k, hipStreamNonBlocking));
    CSDR_HIP(hipStreamCreateWithFlags(&h->s_out, hipStreamNonBlocking));
    for (auto &sl : h->slot) {
        CSDR_HIP(hipEventCreateWithFlags(&sl.e_in, hipEventDisableTiming));
        CSDR_HIP(hipEventCreateWithFlags(&sl.e_k, hipEventDisableTiming));
        CSDR_HIP(hipEventCreateWithFlags(&sl.e_out, hipEventDisableTiming));
    }
    return CSDR_OK;
}

int csdr_chain_submit(csdr_chain *h, const float *in, uint32_t n_in, void *out)
{
    if (!h) { set_error("chain: null handle"); return CSDR_ERR_INVALID; }
    DevGuard guard;
    int r;
    if ((r = chain_check_chunk(h, in, n_in, out, guard))) return r;
    if (h->q_count == CSDR_CHAIN_INFLIGHT) { set_error("chain: %d chunks already in flight (collect first)", CSDR_CHAIN_INFLIGHT); return CSDR_ERR_BUSY; }
    if ((r = chain_host_init(h))) return r;
    if (h->user_stream_dirty) {                         // csdr_chain_process_device calls on caller streams precede this chunk
        CSDR_HIP(hipEventSynchronize(h->e_user));
        h->user_stream_dirty = false;
    }
    csdr_chain::HostSlot &sl = h->slot[(h->q_head + h->q_count) % CSDR_CHAIN_INFLIGHT];
    sl.user_out = out; sl.n_out = 0; sl.out_bytes = 0; sl.staged_out = false;
    if (n_in) {
        const size_t in_bytes = sizeof(float2) * (size_t)n_in, out_max = (size_t)h->C * h->max_nf * 8;
        if (!sl.d_in && ((r = chain_alloc(h, &sl.d_in, h->max_nx)))) return r;
        if (!sl.d_out) { CSDR_HIP(hipMalloc(&sl.d_out, out_max)); }
        // every resource of the slot exists before the chain's state moves on: a failure below this point cannot skip a chunk's state
        const bool stage_out = !is_pinned(out);
        if (stage_out && !sl.h_out) { CSDR_HIP(hipHostMalloc(&sl.h_out, out_max, hipHostMallocDefault)); }
        const void *src = in;
        if (!is_pinned(in)) {                               // pageable caller memory: one host copy into the slot's page-locked buffer
            if (!sl.h_in) { CSDR_HIP(hipHostMalloc(&sl.h_in, sizeof(float2) * h->max_nx, hipHostMallocDefault)); }
            memcpy(sl.h_in, in, in_bytes);
            src = sl.h_in;
        }
        CSDR_HIP(hipMemcpyAsync(sl.d_in, src, in_bytes, hipMemcpyHostToDevice, h->s_in));
        CSDR_HIP(hipEventRecord(sl.e_in, h->s_in));
        CSDR_HIP(hipStreamWaitEvent(h->s_k, sl.e_in, 0));
        // the slot's device output was last read by its own previous D2H copy
        CSDR_HIP(hipStreamWaitEvent(h->s_k, sl.e_out, 0));
        uint32_t no = 0;
        if ((r = csdr_chain_process_device(h, sl.d_in, n_in, sl.d_out, &no, h->s_k))) return r;
        CSDR_HIP(hipEventRecord(sl.e_k, h->s_k));
        sl.n_out = no; sl.out_bytes = (size_t)no * csdr_chain_out_elem_size(h);
        void *dst = out;
        if (stage_out) { dst = sl.h_out; sl.staged_out = true; }
        CSDR_HIP(hipStreamWaitEvent(h->s_out, sl.e_k, 0));
        CSDR_HIP(hipMemcpyAsync(dst, sl.d_out, sl.out_bytes, hipMemcpyDeviceToHost, h->s_out));
        CSDR_HIP(hipEventRecord(sl.e_out, h->s_out));
    }
    h->q_count++;
    return CSDR_OK;
}

int csdr_chain_collect(csdr_chain *h, uint32_t *n_out)
{
    if (!h) { set_error("chain: null handle"); return CSDR_ERR_INVALID; }
    if (n_out) *n_out = 0;
    if (!h->q_count) { set_error("chain: nothing submitted"); return CSDR_ERR_INVALID; }
    DevGuard guard(h->device);
    csdr_chain::HostSlot &sl = h->slot[h->q_head];
    if (sl.out_bytes) {
        CSDR_HIP(hipEventSynchronize(sl.e_out));        // (a failed wait leaves the chunk queued)
        if (sl.staged_out) memcpy(sl.user_out, sl.h_out, sl.out_bytes);
    }
    h->q_head = (h->q_head + 1) % CSDR_CHAIN_INFLIGHT; h->q_count--;
    if (n_out) *n_out = sl.n_out;
    return CSDR_OK;
}

int csdr_chain_process(csdr_chain *h, const float *in, uint32_t n_in, void *out, uint32_t *n_out)
{
    if (!h) { set_error("chain: null handle"); return CSDR_ERR_INVALID; }
    if (n_out) *n_out = 0;
    if (n_in == 0) return CSDR_OK;
    if (h->q_count) { set_error("chain: csdr_chain_process with chunks still in flight (collect them first)"); return CSDR_ERR_BUSY; }
    int r;
    if (is_pinned(in) && is_pinned(out)) {
        if ((r = csdr_chain_submit(h, in, n_in, out))) return r;
        if ((r = csdr_chain_collect(h, n_out))) return r;
    } else {
        // pageable caller memory: the runtime's own staged hipMemcpy beats a hand-made copy into page-locked memory
        DevGuard guard;
        if ((r = chain_check_chunk(h, in, n_in, out, guard))) return r;
        if ((r = chain_host_init(h))) return r;
        if (h->user_stream_dirty) { CSDR_HIP(hipEventSynchronize(h->e_user)); h->user_stream_dirty = false; }
        csdr_chain::HostSlot &sl = h->slot[0];
        if (!sl.d_in && ((r = chain_alloc(h, &sl.d_in, h->max_nx)))) return r;
        if (!sl.d_out) { CSDR_HIP(hipMalloc(&sl.d_out, (size_t)h->C * h->max_nf * 8)); }
        CSDR_HIP(hipMemcpy(sl.d_in, in, sizeof(float2) * (size_t)n_in, hipMemcpyHostToDevice));
        uint32_t no = 0;
        if ((r = csdr_chain_process_device(h, sl.d_in, n_in, sl.d_out, &no, h->s_k))) return r;
        CSDR_HIP(hipStreamSynchronize(h->s_k));
        CSDR_HIP(hipMemcpy(out, sl.d_out, (size_t)no * csdr_chain_out_elem_size(h), hipMemcpyDeviceToHost));
        if (n_out) *n_out = no;
    }
    if ((r = chain_device_status(h))) return r;
    return CSDR_OK;
}

int csdr_chain_reset(csdr_chain *h)
{
    if (!h) return CSDR_ERR_INVALID;
    DevGuard guard(h->device);
    CSDR_HIP(hipDeviceSynchronize());                  // chunks still in flight are abandoned
    h->q_head = 0; h->q_count = 0;
    h->pd_used[0] = h->pd_used[1] = false; h->pd_tail_rec = false; h->serial_pending = false; h->pd_count = 0;
    h->user_stream_dirty = false; h->pd_last_indep = false;
    int r = chain_init_state(h, nullptr);
    if (r) return r;
    CSDR_HIP(hipDeviceSynchronize());
    return chain_device_status(h);
}

int csdr_chain_seek_frames(csdr_chain *h, uint64_t frames)
{
    int r = csdr_chain_reset(h);
    if (r) return r;
    h->theta = (uint32_t)(frames * (uint64_t)h->M * (uint64_t)h->d_theta);
    if (h->plan) h->plan->seek(frames);
    return CSDR_OK;
}

int csdr_chain_get_taps(const csdr_chain *h, float *taps, uint32_t n)
{
    if (!h || !taps) return CSDR_ERR_INVALID;
    if (n > h->taps.size()) n = (uint32_t)h->taps.size();
    memcpy(taps, h->taps.data(), sizeof(float) * n);
    return (int)n;
}
int csdr_chain_get_nco(const csdr_chain *h, uint32_t *theta, uint32_t *d_theta)
{
    if (!h) return CSDR_ERR_INVALID;
    if (theta) *theta = h->theta;
    if (d_theta) *d_theta = h->d_theta;
    return CSDR_OK;
}
int csdr_chain_debug_trace(csdr_chain *h, unsigned long long *out, uint32_t ntiles)
{
    if (!h || !out) return CSDR_ERR_INVALID;
    return h->plan ? h->plan->trace(out, ntiles) : 0;
}
int csdr_chain_debug_agc(csdr_chain *h, uint32_t *checked, uint32_t *redone)
{
    if (!h) return CSDR_ERR_INVALID;
    if (checked) *checked = 0;
    if (redone) *redone = 0;
    if (!h->agc_tail) return 0;
    DevGuard guard(h->device);
    (void)hipDeviceSynchronize();
    return agc_tail_stats(h->agc_tail, checked, redone);
}
uint32_t csdr_chain_debug_agc_tile_major_calls(const csdr_chain *h) { return h && h->agc_tail ? agc_tail_tm_calls(h->agc_tail) : 0u; }
const char *csdr_chain_path(const csdr_chain *h) { return h ? h->path.c_str() : ""; }
int csdr_chain_get_cfg(const csdr_chain *h, csdr_chain_cfg *cfg_out)
{
    if (!h || !cfg_out) { set_error("csdr_chain_get_cfg: null argument"); return CSDR_ERR_INVALID; }
    *cfg_out = h->cfg;
    return CSDR_OK;
}

const char *csdr_chain_kernel_time(csdr_chain *h, double *total_ms, uint32_t *launches)
{
    if (!h) return "";
    if (h->s_pd[0] && h->timer.region && h->timer.open && h->timer.last) {
        DevGuard guard(h->device);
        for (int i = 0; i < 2; i++) if (h->pd_used[i]) (void)hipStreamWaitEvent(h->timer.last, h->e_pd_done[i], 0);
    }
    (void)h->timer.drain();
    if (total_ms) *total_ms = h->timer.acc_ms;
    if (launches) *launches = h->timer.launches;
    h->timer.acc_ms = 0.0; h->timer.launches = 0;
    return h->plan ? h->plan->name() : "k_agc_spec";      // the kernel the last call timed (before the first call: the create-time choice)
}

int csdr_chain_destroy(csdr_chain *h)
{
    if (!h) return CSDR_OK;
    DevGuard guard(h->device);
    (void)hipDeviceSynchronize();
    delete h->plan;
    if (h->agc_tail) agc_tail_destroy(h->agc_tail);
    h->timer.destroy();
    for (auto &sl : h->slot) {
        if (sl.d_out) (void)hipFree(sl.d_out);
        if (sl.h_in) (void)hipHostFree(sl.h_in);
        if (sl.h_out) (void)hipHostFree(sl.h_out);
        for (hipEvent_t e : {sl.e_in, sl.e_k, sl.e_out}) if (e) (void)hipEventDestroy(e);
    }
    for (hipStream_t st : {h->s_in, h->s_k, h->s_out, h->s_pd[0], h->s_pd[1]}) if (st) (void)hipStreamDestroy(st);
    for (hipEvent_t e : {h->e_pd_done[0], h->e_pd_done[1], h->e_pd_tail[0], h->e_pd_tail[1], h->e_pd_tail[2], h->e_serial, h->e_user}) if (e) (void)hipEventDestroy(e);
    delete h;
    return CSDR_OK;
}

}  // extern "C"

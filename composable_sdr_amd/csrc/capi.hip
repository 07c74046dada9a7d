// C ABI of libcsdr_hip.so (see include/csdr.h): the route table and the chain handle (the plan of its route, the tails behind
// it (chain_tails.h), stream state and the per-chunk call sequence).  The handles of the single blocks are in capi_blocks.hip.  Product code: no CPU fallback,
// nothing from oracle/.
#include "../../include/csdr.h"
#include "capi_internal.h"
#include "chain_tails.h"
#include "fused.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

namespace csdr {
const char *last_error();
}
using namespace csdr;

struct csdr_chain {
    // what mem and the members' own destructors do not release (block_destroy: the device is selected and idle)
    ~csdr_chain()
    {
        delete plan;
        timer.destroy();
        for (hipStream_t st : {s_in, s_k, s_out}) if (st) (void)hipStreamDestroy(st);
        if (e_user) (void)hipEventDestroy(e_user);
    }
    csdr_chain_cfg cfg;
    int device = -1;
    uint32_t M = 0, p = 0, C = 0, c0 = 0, max_nf = 0; uint64_t max_nx = 0;
    uint32_t G = 1;                  // chan_stride: interleaved shard g = c0 of G
    std::string path;
    // design
    std::vector<float> taps;
    uint32_t theta = 0, d_theta = 0;
    DeviceBuffers mem;               // the handle's device memory, the tails' and the slots' included
    ChainPlan *plan = nullptr;       // the route's plan (fused.h); null: CSDR_FLAG_TAIL_ONLY, the caller's rows are the front
    std::unique_ptr<AgcTail> agc;    // AGC on
    std::unique_ptr<AmTail> am;
    std::unique_ptr<WbfmTail> wbfm;
    std::unique_ptr<RowReversal> backward;
    KernelTimer timer;
    // host-API staging: CSDR_CHAIN_INFLIGHT slots (device in / out, page-locked host in / out), three streams
    struct HostSlot {
        ~HostSlot()
        {
            for (void *q : {h_in, h_out}) if (q) (void)hipHostFree(q);
            for (hipEvent_t e : {e_in, e_k, e_out}) if (e) (void)hipEventDestroy(e);
        }
        float2 *d_in = nullptr; void *d_out = nullptr; void *h_in = nullptr, *h_out = nullptr;
        hipEvent_t e_in = nullptr, e_k = nullptr, e_out = nullptr;
        void *user_out = nullptr; uint32_t n_out = 0; size_t out_bytes = 0; bool staged_out = false;
    };
    HostSlot slot[CSDR_CHAIN_INFLIGHT];
    hipStream_t s_in = nullptr, s_k = nullptr, s_out = nullptr;
    uint32_t q_head = 0, q_count = 0;      // oldest pending slot, number of pending chunks
    // pipelined device entry point (csdr_chain_submit_device; made by its first call): two handle-owned streams used alternately, so
    // that consecutive chunks' launches may overlap (the next launch's cold run starts fill the CUs the previous one has already left)
    struct Pipelined {
        ~Pipelined()
        {
            for (hipStream_t q : s) if (q) (void)hipStreamDestroy(q);
            for (hipEvent_t e : {e_done[0], e_done[1], e_tail[0], e_tail[1], e_tail[2], e_serial}) if (e) (void)hipEventDestroy(e);
        }
        int open()
        {
            bool ok = true;
            for (hipStream_t &q : s) ok = ok && hipStreamCreateWithFlags(&q, hipStreamNonBlocking) == hipSuccess;
            for (hipEvent_t *e : {&e_done[0], &e_done[1], &e_tail[0], &e_tail[1], &e_tail[2], &e_serial})
                ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
            if (ok) return CSDR_OK;
            (void)hipGetLastError();
            set_error("chain: cannot create the streams / events of the pipelined entry point");
            return CSDR_ERR_HIP;
        }
        void reset() { used[0] = used[1] = tail_rec = serial_pending = last_indep = false; count = 0; }     // chunks in flight are abandoned
        hipStream_t s[2] = {nullptr, nullptr};
        hipEvent_t e_done[2] = {nullptr, nullptr}, e_tail[3] = {nullptr, nullptr, nullptr}, e_serial = nullptr;
        bool used[2] = {false, false}, tail_rec = false, serial_pending = false;
        bool last_indep = false;         // the previous csdr_chain_submit_device call ran as an independent launch
        uint32_t count = 0, indep_calls = 0;
    };
    std::unique_ptr<Pipelined> pd;
    // entry points share the handle's state: a call on a caller's stream is remembered so that the host-buffer entry point
    // (own stream s_k) can order itself behind it, and the other way round
    // (a handle-owned event recorded on the caller's stream behind the call's work: the caller may destroy the stream afterwards)
    hipEvent_t e_user = nullptr; bool user_stream_dirty = false;
};
using HostSlot = csdr_chain::HostSlot;

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
    h->theta = 0;
    int r;
    if (h->agc && (r = h->agc->reset(s))) return r;
    if (h->am && (r = h->am->reset(s))) return r;
    if (h->wbfm && (r = h->wbfm->reset(s))) return r;
    return h->plan ? h->plan->reset(s) : 0;
}

// argument checks -> device -> handle -> design -> front (the route's plan; CSDR_FLAG_TAIL_ONLY: none) -> tails -> state -> print
int csdr_chain_create(const csdr_chain_cfg *cfg_in, csdr_chain **out)
{
    if (!cfg_in || !out) { set_error("chain: null argument"); return CSDR_ERR_INVALID; }
    if (cfg_in->struct_size != sizeof(csdr_chain_cfg)) { set_error("chain: cfg.struct_size %u != %zu", cfg_in->struct_size, sizeof(csdr_chain_cfg)); return CSDR_ERR_INVALID; }
    if (cfg_in->demod > CSDR_DEMOD_WBFM) { set_error("chain: unknown demod %u", cfg_in->demod); return CSDR_ERR_INVALID; }
    // DeAM = amDemodulator . agc (SoapySDR.hs:265-272): everything up to the per-channel CF32 samples is the DeNo
    // chain; the peak detector and the mix follow as a tail (AmTail)
    csdr_chain_cfg eff = *cfg_in;
    const bool am = cfg_in->demod == CSDR_DEMOD_AM, wbfm = cfg_in->demod == CSDR_DEMOD_WBFM, tail_mix = cfg_in->mix != 0 && cfg_in->channels > 1;
    if (am) { eff.demod = CSDR_DEMOD_NONE; eff.mix = 0; }
    // DeWBFM decim = firDecimator decim . iirDeemph . fmDemodulator 0.6 . agc (SoapySDR.hs:252-259, Liquid.chs:653-656)
    if (wbfm) { eff.demod = CSDR_DEMOD_FM; eff.kf = 0.6f; eff.mix = 0; }
    const csdr_chain_cfg *cfg = &eff;
    if (cfg->channels < 1 || cfg->channels > (1u << 16)) { set_error("chain: channels %u out of range", cfg->channels); return CSDR_ERR_INVALID; }
    // CSDR_FLAG_TAIL_ONLY: the per-channel tail alone (hybrid multi-GPU partition): rows in, rows out, no plan
    const bool tail_only = (cfg_in->flags & CSDR_FLAG_TAIL_ONLY) != 0, agc_on = cfg->agc_threshold_db != 0.0f;
    if (tail_only && (!agc_on || am || wbfm)) { set_error("chain: CSDR_FLAG_TAIL_ONLY needs the AGC on (-a != 0) and demod none / FM (without the AGC a time stripe needs no tail shard)"); return CSDR_ERR_INVALID; }
    if (cfg->demod == CSDR_DEMOD_FM && !(cfg->kf > 0.f)) { set_error("chain: FM needs kf > 0"); return CSDR_ERR_INVALID; }
    const uint32_t M = cfg->channels, G = !tail_only && cfg->chan_stride > 1 ? cfg->chan_stride : 1;
    uint32_t c0 = 0, C = M;
    if (tail_only) { eff.chan_first = 0; eff.chan_count = 0; eff.chan_stride = 0; eff.dc_block = 0; }
    else {
        if (cfg->dc_block && !(cfg->dc_alpha > 0.f && cfg->dc_alpha < 1.f)) { set_error("chain: dc_alpha out of (0,1)"); return CSDR_ERR_INVALID; }
        if (cfg->pfb_m > 32u) { set_error("chain: pfb_m %u out of 1..32 (0 = 7)", cfg->pfb_m); return CSDR_ERR_INVALID; }
        c0 = cfg->chan_first; C = cfg->chan_count ? cfg->chan_count : M - c0;
        if (G > 1) {
            if (M % G || c0 >= G || (cfg->chan_count && cfg->chan_count != M / G)) {
                set_error("chain: interleaved shard %u of %u needs chan_stride | channels (%u), chan_first < chan_stride, chan_count 0 or channels/chan_stride", c0, G, M);
                return CSDR_ERR_INVALID;
            }
            C = M / G;
        } else if (c0 >= M || C == 0 || c0 + C > M) { set_error("chain: channel shard [%u,+%u) outside 0..%u", c0, C, M); return CSDR_ERR_INVALID; }
    }
    NewBlock<csdr_chain> nb;
    int r = nb.open(cfg->device); if (r) return r;
    csdr_chain *h = nb.get();
    DevGuard guard(h->device);
    if (!guard.ok) { set_error("chain: cannot select device %d", h->device); return CSDR_ERR_HIP; }

    const uint32_t m = cfg->pfb_m ? cfg->pfb_m : 7;
    const float As = cfg->pfb_as > 0.f ? cfg->pfb_as : 80.0f;
    h->cfg = *cfg; h->M = M; h->C = C; h->c0 = c0; h->G = G; h->p = tail_only ? 0 : 2 * m;
    h->max_nf = cfg->max_frames ? cfg->max_frames : 4096;
    h->max_nx = (uint64_t)h->max_nf * M;
    if (h->max_nx > 0xffffffffull) { set_error("chain: max_frames*channels exceeds 2^32-1 samples"); return CSDR_ERR_INVALID; }

    // Front.  With the AGC on, the plan stops at the channel-major CF32 samples and the per-channel AGC tail (time-parallel, or
    // with CSDR_FLAG_AGC_SEQUENTIAL one lane per channel) + freqdem + mix follow.
    const RouteRow *route = nullptr;
    std::string front = "tail-only+agc";
    int cus = 256;                   // compute units of the device (run counts of k_pfb1024 and of the plans: FusedConfig::cus; the AGC tail's segments)
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device);
    if (!tail_only) {
        h->timer.enabled = (cfg->flags & (CSDR_FLAG_TIME_KERNELS | CSDR_FLAG_TIME_REGION)) != 0;
        h->timer.region = (cfg->flags & CSDR_FLAG_TIME_REGION) != 0;
        DcParams dc{};
        if (cfg->dc_block) dc = make_dc(cfg->dc_alpha);
        if (M > 1) {
            h->taps = design_pfb_taps(M, m, As);
            h->d_theta = nco_freq_word(pfb_premix_freq(M));
        }
        // interleaved shards: the fused M = 256 and 1024 chains take strides 2, 4, 8; every other shape the any-M route with a pruned DFT
        const DcParams *dcp = cfg->dc_block ? &dc : nullptr;
        route = route_select(M, h->p, G, cfg->flags, dcp);     // the one place a configuration is mapped to a plan (table above)
        if (route->M == 4096 && (C != M || (cfg->mix && cfg->demod == CSDR_DEMOD_NONE && !agc_on && !am)))
            route = route_select(M, h->p, G, cfg->flags | CSDR_FLAG_FORCE_GENERIC, dcp);   // contiguous shards; DeNo --mix over all channels (= M x branch 0: nothing beats not computing
                                                                                       // the bank; CSDR_FLAG_NO_MIX_IDENTITY's full bank + DFT + sum stays on the any-M kernels too)
        FusedConfig fc{};
        fc.M = M; fc.p = h->p; fc.C = C; fc.c0 = c0; fc.max_nf = h->max_nf; fc.G = G;
        fc.dc_block = cfg->dc_block != 0; fc.dc = dc;
        fc.fm = cfg->demod == CSDR_DEMOD_FM && !agc_on; fc.fm_ref = cfg->demod == CSDR_DEMOD_FM ? fm_ref_of(cfg->kf) : 0.f;     // (with the AGC on its tail does the freqdem)
        fc.mix = cfg->mix != 0 && !agc_on; fc.taps = h->taps.data(); fc.d_theta = h->d_theta; fc.cus = (uint32_t)cus;
        fc.no_mix_identity = (cfg->flags & CSDR_FLAG_NO_MIX_IDENTITY) != 0;
        if ((r = route->create(fc, &h->plan))) return r;
        front = h->plan->route(route->path_prefix, agc_on);
    }
    h->path = front;

    // Tails (the order of their checks is part of the C ABI; the AGC tail's piece of the path comes last)
    const bool fused = route && route->M;
    if (agc_on) {
        h->agc = std::make_unique<AgcTail>();
        if ((r = h->agc->setup(h->mem, *cfg, C, h->max_nf, !tail_only, fused, (uint32_t)cus))) return r;
    }
    if (!tail_only && (cfg_in->flags & CSDR_FLAG_DFT_BACKWARD) && M > 1 && !(cfg_in->mix != 0)) {
        if (C != M || G > 1) { set_error("chain: CSDR_FLAG_DFT_BACKWARD is built for whole-band handles (no channel shard)"); return CSDR_ERR_INVALID; }
        h->backward = std::make_unique<RowReversal>();
        if ((r = h->backward->setup(h->mem, C, h->max_nf, cfg_in->demod == CSDR_DEMOD_NONE ? 8u : 4u, h->path))) return r;
    }
    if (am) {
        h->am = std::make_unique<AmTail>();
        if ((r = h->am->setup(h->mem, C, h->max_nf, tail_mix, h->path))) return r;
    }
    if (wbfm) {
        h->wbfm = std::make_unique<WbfmTail>();
        if ((r = h->wbfm->setup(h->mem, *cfg_in, C, h->max_nf, tail_mix, h->path))) return r;
    }
    if (h->agc) h->path += h->agc->path_piece();
    if ((r = chain_init_state(h, nullptr))) return r;
    CSDR_HIP(hipDeviceSynchronize());

    if (!(cfg->flags & CSDR_FLAG_QUIET)) {
        const char *demod = am ? "AM" : (wbfm ? "WBFM" : (cfg->demod == CSDR_DEMOD_FM ? "FM" : "none"));
        // what the reference prints at create (Liquid.chs:577-579, 814-820, 714-716, 319-321)
        if (tail_only)
            printf("csdr chain [%s] on HIP device %d: %u channel rows, agc=%g dB demod=%s kf=%g mix=%u\n", h->path.c_str(), h->device, h->C,
                   cfg->agc_threshold_db, demod, cfg->kf, cfg->mix);
        else
            printf("csdr chain [%s] on HIP device %d: channels=%u (shard %u..%u) taps=%u (m=%u, As=%.1f) "
                   "nco.d_theta=0x%08x dc_block=%u(alpha=%g) agc=%g dB demod=%s kf=%g mix=%u\n",
                   h->path.c_str(), h->device, M, c0, c0 + C - 1, M > 1 ? M * h->p : 0, m, As, h->d_theta, cfg->dc_block,
                   cfg->dc_alpha, cfg->agc_threshold_db, demod, cfg->kf, cfg_in->mix);
        // per-channel outputs / AGC / demod tails beyond the fused kernels' channel counts run stage by stage through HBM
        if (route && !route->M && M > 1024 && front != "generic+mix-identity")
            printf("csdr chain: note: %u channels with per-channel output run on the any-M route (DC blocker, FIR, DFT and tail as separate kernels, "
                   "~0.09 of the HBM roofline on MI355X); fused kernels exist for 64, 256 and 1024 channels, and for DeNo --mix over all channels of any count\n", M);
        fflush(stdout);
    }
    return nb.publish(out);
}

uint32_t csdr_chain_out_elem_size(const csdr_chain *h) { return h && (h->cfg.demod == CSDR_DEMOD_FM || h->am || h->wbfm) ? 4u : 8u; }

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

// One call on s: the plan (tail-only: the caller's rows), the AGC tail, the AM or the WBFM tail, the backward handle's row
// reversal.  Every stage writes the next stage's input, the last one d_out.  indep, ev_tail: csdr_chain_submit_device's, for the plan
static int chain_call(csdr_chain *h, const void *d_in, uint32_t n_in, void *d_out, uint32_t *n_out, hipStream_t s, bool indep = false,
                      hipEvent_t ev_tail = nullptr)
{
    // 1. checks (texts, codes and their order are part of the C ABI)
    const bool backward = h->backward && n_in && d_out;         // (with nothing to do or nowhere to put it a backward handle answers as a forward one)
    if (n_out && !backward) *n_out = 0;                         // (a call a backward handle refuses has always left *n_out alone)
    if (n_in == 0) return CSDR_OK;
    if (!d_out) { set_error("chain: null buffer"); return CSDR_ERR_INVALID; }
    if (h->wbfm && n_in % h->M == 0 && (n_in / h->M) % h->wbfm->decim()) {
        set_error("chain: %u frames per call are not a multiple of the WBFM decimation %u (firDecim's `div`, Liquid.chs:495-497)", n_in / h->M, h->wbfm->decim());
        return CSDR_ERR_SIZE;
    }
    DevGuard guard;
    int r;
    if ((r = chain_check_chunk(h, d_in, n_in, d_out, guard))) return r;
    const uint32_t nf = n_in / h->M, C = h->C;
    const bool fm = h->cfg.demod == CSDR_DEMOD_FM, mixo = h->cfg.mix && h->M > 1;
    void *const last = backward ? h->backward->input() : d_out;                                   // output of stage 4
    void *const chain_out = h->wbfm ? h->wbfm->input() : h->am ? h->am->input() : last;           // output of stages 2 + 3
    uint32_t n = mixo ? nf : C * nf;                                                              // elements in it

    // 2. front: the route's plan writes Z: chain_out, or with the AGC on the plane its tail reads (chain_out itself where the sequential
    // AGC is the last step and works in place).  Tail-only: Z = the caller's rows (the sequential AGC works in place on a copy)
    float2 *Z;
    bool tm = false;
    if (h->plan) {
        FusedCall fcall{};
        Z = h->agc ? h->agc->plane(chain_out) : (float2 *)chain_out;
        // time-parallel AGC tail behind a fused plan, run-sized calls of whole tiles: the plane between the two kernels is tile-major
        tm = h->agc && h->agc->tile_major(nf) && h->plan->tile_major_ok(nf);
        fcall.tile_major = tm;
        fcall.d_in = (const float2 *)d_in; fcall.d_out = Z; fcall.nf = nf; fcall.theta0 = h->theta;
        fcall.indep = indep; fcall.ev_tail = ev_tail;
        if ((r = h->plan->process(fcall, s, &h->timer))) return r;
        h->theta += n_in * h->d_theta;     // the NCO phase behind the call
    } else if (h->agc->time_parallel()) Z = (float2 *)d_in;
    else { Z = h->agc->plane(chain_out); CSDR_HIP(hipMemcpyAsync(Z, d_in, sizeof(float2) * (size_t)n_in, hipMemcpyDeviceToDevice, s)); }

    // 3. AGC + squelch [+ freqdem] [+ mix]
    if (h->agc && (r = h->agc->run(Z, nf, chain_out, s, tm))) return r;
    if (!h->plan && !h->agc->time_parallel() && !fm && !mixo) CSDR_HIP(hipMemcpyAsync(chain_out, Z, sizeof(float2) * (size_t)n_in, hipMemcpyDeviceToDevice, s));

    // 4. DeWBFM: the chain ran as DeNBFM 0.6; de-emphasis + decimator [+ mix].  DeAM: it ran as DeNo; the ampmodem peak detector [+ mix]
    if (h->wbfm && (r = h->wbfm->run(nf, last, &n, s))) return r;
    if (h->am && (r = h->am->run(nf, last, &n, s))) return r;
    if (n_out) *n_out = n;

    // 5. CSDR_FLAG_DFT_BACKWARD: the chain as built (forward DFT) went into last; row k of the output = its row (M - k) mod M
    return backward ? h->backward->run(n, d_out, s) : CSDR_OK;
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
    if (!h) { set_error("chain: null handle"); return CSDR_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    const bool own = h->s_k && s == h->s_k;             // called by csdr_chain_submit / csdr_chain_process on the handle's stream
    DevGuard guard(h->device);
    if (!own && h->s_k && h->q_count) CSDR_HIP(hipStreamSynchronize(h->s_k));   // host-buffer chunks still in flight come first
    if (h->pd) {
        // the handle has pipelined chunks (csdr_chain_submit_device): this call follows them, and a later submit follows this call
        for (int i = 0; i < 2; i++) if (h->pd->used[i]) CSDR_HIP(hipStreamWaitEvent(s, h->pd->e_done[i], 0));
    }
    int r = chain_call(h, d_in, n_in, d_out, n_out, s);
    if (r) return r;
    if (h->pd) {
        CSDR_HIP(hipEventRecord(h->pd->e_serial, s));
        h->pd->serial_pending = true;
    }
    return own ? CSDR_OK : chain_mark_user_stream(h, s);
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
    if (!h->pd) {
        CSDR_HIP(hipDeviceSynchronize());               // whatever the handle has queued on caller streams so far
        // made apart and published whole: a partial failure leaves the handle as it was
        auto pd = std::make_unique<csdr_chain::Pipelined>();
        if (int r = pd->open()) return r;
        h->pd = std::move(pd);
        if (h->plan) h->plan->keep_tail();
    }
    csdr_chain::Pipelined &pd = *h->pd;
    if (h->s_k && h->q_count) CSDR_HIP(hipStreamSynchronize(h->s_k));       // host-buffer chunks still in flight come first
    const uint32_t nf = n_in / h->M, k = pd.count;
    const int si = (int)(k & 1);
    hipStream_t s = pd.s[si];
    // An independent launch (fused M = 256 chain without AGC / AM / WBFM tails, run-kernel-sized whole-tile chunk, previous
    // chunk's tail on file) reads nothing an earlier launch writes: it only waits for the input and for the copy of the
    // previous chunk's tail.  Every other call is ordered behind everything the handle has in flight.
    const bool overlap = h->plan && !h->agc && !h->am && !h->wbfm && h->plan->can_overlap(nf);
    if (ready_event) CSDR_HIP(hipStreamWaitEvent(s, (hipEvent_t)ready_event, 0));
    if (pd.serial_pending) { CSDR_HIP(hipStreamWaitEvent(s, pd.e_serial, 0)); pd.serial_pending = false; }
    if (overlap) {
        if (pd.tail_rec) CSDR_HIP(hipStreamWaitEvent(s, pd.e_tail[(k + 2) % 3], 0));       // recorded by call k - 1
        // a call k - 1 that was NOT independent reads the plan's ping-pong state (run 0) that this launch's last run overwrites:
        // then this launch follows all of it, not only its tail copy
        if (!pd.last_indep && pd.used[si ^ 1]) CSDR_HIP(hipStreamWaitEvent(s, pd.e_done[si ^ 1], 0));
    } else if (pd.used[si ^ 1]) CSDR_HIP(hipStreamWaitEvent(s, pd.e_done[si ^ 1], 0));
    if (int r = chain_call(h, d_in, n_in, d_out, n_out, s, overlap, pd.e_tail[k % 3])) return r;
    pd.tail_rec = h->plan && h->plan->tail_recorded();
    if (overlap) pd.indep_calls++;
    pd.last_indep = overlap;
    CSDR_HIP(hipEventRecord(pd.e_done[si], s));
    pd.used[si] = true; pd.count = k + 1;
    return CSDR_OK;
}

uint32_t csdr_chain_debug_independent_launches(const csdr_chain *h) { return h && h->pd ? h->pd->indep_calls : 0u; }

int csdr_chain_wait_device(csdr_chain *h, void *stream)
{
    if (!h) { set_error("chain: null handle"); return CSDR_ERR_INVALID; }
    DevGuard guard(h->device);
    for (int i = 0; h->pd && i < 2; i++) {
        if (!h->pd->used[i]) continue;
        if (stream) CSDR_HIP(hipStreamWaitEvent((hipStream_t)stream, h->pd->e_done[i], 0));
        else CSDR_HIP(hipEventSynchronize(h->pd->e_done[i]));
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

// What a host-buffer call of n_in samples through slot sl needs first: the handle's streams and events, the calls on caller
// streams behind it, the slot's device buffers
static int chain_slot_setup(csdr_chain *h, HostSlot &sl, uint32_t n_in)
{
    int r;
    if ((r = chain_host_init(h))) return r;
    if (h->user_stream_dirty) {                         // csdr_chain_process_device calls on caller streams precede this chunk
        CSDR_HIP(hipEventSynchronize(h->e_user));
        h->user_stream_dirty = false;
    }
    if (n_in && !sl.d_in && (r = h->mem.alloc_n(&sl.d_in, h->max_nx))) return r;
    if (n_in && !sl.d_out && (r = h->mem.alloc(&sl.d_out, (size_t)h->C * h->max_nf * 8))) return r;
    return CSDR_OK;
}

int csdr_chain_submit(csdr_chain *h, const float *in, uint32_t n_in, void *out)
{
    if (!h) { set_error("chain: null handle"); return CSDR_ERR_INVALID; }
    DevGuard guard;
    int r;
    if ((r = chain_check_chunk(h, in, n_in, out, guard))) return r;
    if (h->q_count == CSDR_CHAIN_INFLIGHT) { set_error("chain: %d chunks already in flight (collect first)", CSDR_CHAIN_INFLIGHT); return CSDR_ERR_BUSY; }
    HostSlot &sl = h->slot[(h->q_head + h->q_count) % CSDR_CHAIN_INFLIGHT];
    if ((r = chain_slot_setup(h, sl, n_in))) return r;
    sl.user_out = out; sl.n_out = 0; sl.out_bytes = 0; sl.staged_out = false;
    if (n_in) {
        const size_t in_bytes = sizeof(float2) * (size_t)n_in, out_max = (size_t)h->C * h->max_nf * 8;
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
    HostSlot &sl = h->slot[h->q_head];
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
        HostSlot &sl = h->slot[0];
        if ((r = chain_slot_setup(h, sl, n_in))) return r;
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
    if (h->pd) h->pd->reset();
    h->user_stream_dirty = false;
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
    if (!h->agc || !h->agc->time_parallel()) return 0;
    DevGuard guard(h->device);
    (void)hipDeviceSynchronize();
    return h->agc->stats(checked, redone);
}
uint32_t csdr_chain_debug_agc_tile_major_calls(const csdr_chain *h) { return h && h->agc ? h->agc->tile_major_calls() : 0u; }
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
    if (h->pd && h->timer.region && h->timer.open && h->timer.last) {
        DevGuard guard(h->device);
        for (int i = 0; i < 2; i++) if (h->pd->used[i]) (void)hipStreamWaitEvent(h->timer.last, h->pd->e_done[i], 0);
    }
    (void)h->timer.drain();
    if (total_ms) *total_ms = h->timer.acc_ms;
    if (launches) *launches = h->timer.launches;
    h->timer.acc_ms = 0.0; h->timer.launches = 0;
    return h->plan ? h->plan->name() : "k_agc_spec";      // the kernel the last call timed (before the first call: the create-time choice)
}

int csdr_chain_destroy(csdr_chain *h) { return block_destroy(h); }

}  // extern "C"

// What the two C-ABI translation units (capi.hip: route table and chain; capi_blocks.hip: the block handles) share, and the
// life-cycle of a block handle ("Adding a block").  Everything here is local to the translation unit that includes it.
#pragma once
#include "../../include/csdr.h"
#include "csdr_internal.h"

#include <cmath>
#include <initializer_list>
#include <new>

namespace csdr {
// ---------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------
namespace {

struct DevGuard {
    int prev = -1; bool ok = true;
    DevGuard() = default;
    explicit DevGuard(int dev) { select(dev); }
    void select(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (dev >= 0 && dev != prev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

int check_device(int32_t want, int *out_dev)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no HIP device visible (hipGetDeviceCount: %s); libcsdr_hip has no CPU fallback",
                  e == hipSuccess ? "0 devices" : hipGetErrorString(e));
        return CSDR_ERR_NODEV;
    }
    int dev = want;
    if (dev < 0) { CSDR_HIP(hipGetDevice(&dev)); }
    if (dev >= n) { set_error("device %d out of range (%d visible)", dev, n); return CSDR_ERR_INVALID; }
    *out_dev = dev;
    return 0;
}

DcParams make_dc(float alpha)
{
    DcParams d;
    d.a1 = -1.0f + alpha;                 // iirfilt_crcf_create_dc_blocker
    d.beta = -d.a1;
    for (int i = 0; i < 9; i++) d.beta_pow_thr[i] = (float)std::pow((double)d.beta, (double)(DC_PER_THREAD << i));
    d.beta_blk = std::pow((double)d.beta, (double)DC_BLOCK);
    d.log2_beta = (float)std::log2((double)d.beta);
    return d;
}

static AgcParams make_agc(float thr_db)
{
    AgcParams p; p.alpha = 0.1f; p.g_thr = agc_gain_threshold(thr_db); p.timeout = 1000u;
    return p;
}

static float fm_ref_of(float kf) { return (float)(1.0 / (2.0 * 3.14159265358979323846 * (double)kf)); }

// ---------------------------------------------------------------------------
// Block handles.  A handle struct H has `int device`, `DeviceBuffers mem` (the owner of all its device memory) and, where it takes
// calls of a bounded size, `uint32_t max_n`; whatever else it owns goes in its destructor.  The error texts are part of the ABI.
// ---------------------------------------------------------------------------
// every csdr_<block>_destroy: NULL is fine; the handle's device is selected and idle while the handle and its memory go
template <class H> int block_destroy(H *h)
{
    if (!h) return CSDR_OK;
    DevGuard guard(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return CSDR_OK;
}

// every csdr_<block>_reset / _rewind: NULL is refused, and the handle's device is selected while block_idle_run puts the state back
template <class Body> int block_idle_run(Body body)
{
    CSDR_HIP(hipDeviceSynchronize());                     // nothing of the caller's is still running on the state
    if (int r = body()) return r;
    CSDR_HIP(hipStreamSynchronize(nullptr));              // what body() queued is done before a stream of the caller's goes on
    return CSDR_OK;
}
template <class H, class Body> int block_reset(H *h, Body body)
{
    if (!h) return CSDR_ERR_INVALID;
    DevGuard guard(h->device);
    return block_idle_run(body);
}

// A handle under construction: open() (behind the create's argument checks) finds the device (want, or -1: the current one) and
// makes the handle, publish() hands it to the caller.  Leaving the create on any other way, a CSDR_HIP included, destroys the
// handle and what it owns
template <class H> struct NewBlock {
    NewBlock() = default;
    NewBlock(const NewBlock &) = delete;
    NewBlock &operator=(const NewBlock &) = delete;
    ~NewBlock() { (void)block_destroy(h); }
    int open(int32_t want = -1)
    {
        int dev; int r = check_device(want, &dev); if (r) return r;
        h = new (std::nothrow) H();
        if (!h) return CSDR_ERR_NOMEM;
        h->device = dev;
        return CSDR_OK;
    }
    H *get() const { return h; }
    H *operator->() const { return h; }
    int publish(H **out) { *out = h; h = nullptr; return CSDR_OK; }
private:
    H *h = nullptr;
};

// n elements owned by mem: a copy of src[n], or zeros
template <class T> int block_upload(DeviceBuffers &mem, T **d, const T *src, size_t n)
{
    int r = mem.alloc_n(d, n); if (r) return r;
    if (n) CSDR_HIP(hipMemcpy(*d, src, sizeof(T) * n, hipMemcpyHostToDevice));
    return CSDR_OK;
}
template <class T> int block_zeros(DeviceBuffers &mem, T **d, size_t n)
{
    int r = mem.alloc_n(d, n); if (r) return r;
    if (n) CSDR_HIP(hipMemset(*d, 0, sizeof(T) * n));
    return CSDR_OK;
}

// State a kernel carries from one call to the next as two arrays of n elements owned by mem (n may be 0): a call reads in() and
// writes the whole of out(), flip() behind the successful launch makes its output the next call's input
template <class T> struct PingPong {
    int alloc(DeviceBuffers &mem, size_t n_)
    {
        n = n_;
        int r = mem.alloc_n(&side[0], n);
        return r ? r : mem.alloc_n(&side[1], n);
    }
    int alloc_zeroed(DeviceBuffers &mem, size_t n_)      // a create's: the state of reset(), in place when the create returns
    {
        int r = alloc(mem, n_);
        if (r || (r = reset(nullptr))) return r;
        CSDR_HIP(hipStreamSynchronize(nullptr));
        return CSDR_OK;
    }
    int reset(hipStream_t s)             // zeros on both sides, back to side 0
    {
        cur = 0;
        for (T *p : side)
            if (n) CSDR_HIP(hipMemsetAsync(p, 0, sizeof(T) * n, s));
        return CSDR_OK;
    }
    const T *in() const { return side[cur]; }
    T *out() const { return side[cur ^ 1]; }
    void flip() { cur ^= 1; }
    int flip_behind(int r) { if (!r) flip(); return r; }        // r: what the launch returned; a refused one leaves the state alone
private:
    T *side[2] = {nullptr, nullptr}; size_t n = 0; int cur = 0;
};

// the size of a call that a create takes for max_samples == 0
inline uint32_t block_max_n(uint32_t max_samples, uint32_t dflt = 4096) { return max_samples ? max_samples : dflt; }
// the CU count that a launch shape is sized by (256 where the device does not say)
inline uint32_t block_cu_count(int device)
{
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    return (uint32_t)cus;
}

inline int block_null_arg(const char *name) { set_error("%s: null argument", name); return CSDR_ERR_INVALID; }
inline int block_check_n(const char *name, uint32_t n, uint32_t max_n)
{
    if (n > max_n) { set_error("%s: %u samples > max %u", name, n, max_n); return CSDR_ERR_SIZE; }
    return CSDR_OK;
}
// the checks in front of a host call of n samples per row from x to y
template <class H> int block_check_call(const char *name, const H *h, const void *x, uint32_t n, const void *y)
{
    if (!h || (n && (!x || !y))) return block_null_arg(name);
    return block_check_n(name, n, h->max_n);
}
// a host entry point selects its handle's device (the device entry points do not: the caller's stream names the device)
inline int block_select(const char *name, DevGuard &guard, int device)
{
    guard.select(device);
    if (!guard.ok) { set_error("%s: cannot select device %d", name, device); return CSDR_ERR_HIP; }
    return CSDR_OK;
}
// a buffer that the first host call that wants it allocates, on the handle's device
template <class T> int block_lazy_alloc(const char *name, int device, DeviceBuffers &mem, T **d, size_t n)
{
    if (*d) return CSDR_OK;
    DevGuard guard;
    int r = block_select(name, guard, device);
    return r ? r : mem.alloc_n(d, n);
}
// the host call on the handle's device: x -> d_in, run() (the device entry point or the launch), then every out that has a
// destination and bytes; block_round_trip is the call with one output
struct BlockOut { void *dst; const void *src; size_t bytes; };
template <class Run>
int block_host_call(const char *name, int device, void *d_in, const void *x, size_t in_bytes, Run run, std::initializer_list<BlockOut> outs)
{
    DevGuard guard;
    int r = block_select(name, guard, device); if (r) return r;
    if (in_bytes) CSDR_HIP(hipMemcpy(d_in, x, in_bytes, hipMemcpyHostToDevice));
    if ((r = run())) return r;
    for (const BlockOut &o : outs)
        if (o.dst && o.bytes) CSDR_HIP(hipMemcpy(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost));
    return CSDR_OK;
}
template <class Run>
int block_round_trip(const char *name, int device, void *d_in, const void *x, size_t in_bytes, const void *d_out, void *y,
                     size_t out_bytes, Run run)
{
    return block_host_call(name, device, d_in, x, in_bytes, run, {{y, d_out, out_bytes}});
}

}  // namespace
}  // namespace csdr

// What the two C-ABI translation units (capi.hip: route table and chain; capi_blocks.hip: the block handles) share, and the
// life-cycle of a block handle ("Adding a block").  Everything here is local to the translation unit that includes it.
#pragma once
#include "../../include/csdr.h"
#include "csdr_internal.h"

#include <cmath>
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

// State a kernel carries from one call to the next as two arrays of n elements owned by mem: a call reads in() and writes out(),
// flip() behind the launch makes its output the next call's input
template <class T> struct PingPong {
    int alloc(DeviceBuffers &mem, size_t n_)
    {
        n = n_;
        int r = mem.alloc_n(&side[0], n);
        return r ? r : mem.alloc_n(&side[1], n);
    }
    int reset(hipStream_t s)             // zeros on both sides, back to side 0
    {
        cur = 0;
        for (T *p : side) CSDR_HIP(hipMemsetAsync(p, 0, sizeof(T) * n, s));
        return CSDR_OK;
    }
    const T *in() const { return side[cur]; }
    T *out() const { return side[cur ^ 1]; }
    void flip() { cur ^= 1; }
private:
    T *side[2] = {nullptr, nullptr}; size_t n = 0; int cur = 0;
};

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
// the host round trip on the handle's device: x -> d_in, run() (the device entry point or the launch), d_out -> y
template <class Run>
int block_round_trip(const char *name, int device, void *d_in, const void *x, size_t in_bytes, const void *d_out, void *y,
                     size_t out_bytes, Run run)
{
    DevGuard guard;
    int r = block_select(name, guard, device); if (r) return r;
    CSDR_HIP(hipMemcpy(d_in, x, in_bytes, hipMemcpyHostToDevice));
    if ((r = run())) return r;
    CSDR_HIP(hipMemcpy(y, d_out, out_bytes, hipMemcpyDeviceToHost));
    return CSDR_OK;
}

}  // namespace
}  // namespace csdr

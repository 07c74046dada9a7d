// C++ host side above the C ABI: the reference's block protocol and stream combinators
// (GHC is not available in this image, and the reference is compiled code, so the host-side
// mirror that ships is C++; composable_sdr_amd/*.py is the same thing for the tests).
//
//   Pipe<A,B>      Types.hs:51-55     { start, process, done } around one native handle
//   compose        Types.hs:93-99     process2 >=> process1, done2 before done1
//   idPipe         Types.hs:101-102   Category id (purePipe id)
//   handlePipe     every block's Pipe: create / destroy / process around one csdr_* handle
//   rowPipe        handlePipe on the channel rows of one chunk (flattenRows, splitRows); rows of unequal length throw
//   unPipe         Types.hs:109-115   create now; (per-array map, cleanup) for the stream side
//   Fold<A>        streamly Fold      step / done
//   addPipe        Types.hs:117-131   downstream start first, then create; done: destroy, then downstream
//   takeNArr       Trans.hs:33-56     pass arrays until n samples, trimming the last one
//   compact        Trans.hs:58-84     emit exactly n, keep the rest, flush the remainder at done
//   distribute_    Trans.hs:106-117   element k of the list to fold k (zip semantics)
//   mix            Trans.hs:119-122   left fold of element-wise +
//   fileSink       Sink.hs:29-34      raw chunk writer
//   readFromFile   Source.chs:259-271 raw CF32 chunks of <= n samples
//   openAudioFile / readFromAudioFile  Source.chs:273-307  a mono WAV / AU file through mixUp pi . realToComplex (FileSource)
#pragma once
#include <algorithm>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <time.h>
#include <unistd.h>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/csdr.h"

namespace csdrhost {

using cf32 = std::complex<float>;
template <class T> using Array = std::vector<T>;

struct CsdrError : std::runtime_error {
    int code;
    CsdrError(int c, const std::string &m) : std::runtime_error("csdr error " + std::to_string(c) + ": " + m), code(c) {}
};
inline void check(int code) { if (code != 0) throw CsdrError(code, csdr_last_error()); }   // Common.hs:32-33 `try`

// ---- Pipe -------------------------------------------------------------------------------
template <class A, class B> struct Pipe {
    std::function<std::shared_ptr<void>()> start;
    std::function<B(void *, const A &)> process;
    std::function<void(void *)> done;
};

template <class A, class B, class C> Pipe<A, C> compose(Pipe<B, C> p1, Pipe<A, B> p2)
{
    struct R { std::shared_ptr<void> r1, r2; };
    Pipe<A, C> p;
    p.start = [=]() { auto r = std::make_shared<R>(); r->r1 = p1.start(); r->r2 = p2.start(); return std::static_pointer_cast<void>(r); };
    p.process = [=](void *r, const A &a) { auto *rr = static_cast<R *>(r); return p1.process(rr->r1.get(), p2.process(rr->r2.get(), a)); };
    p.done = [=](void *r) { auto *rr = static_cast<R *>(r); p2.done(rr->r2.get()); p1.done(rr->r1.get()); };
    return p;
}

// a Pipe without a resource: process = f; idPipe is purePipe id
template <class A, class B, class F> Pipe<A, B> purePipe(F f)
{
    Pipe<A, B> p;
    p.start = []() { return std::shared_ptr<void>(); };
    p.process = [f](void *, const A &a) { return f(a); };
    p.done = [](void *) {};
    return p;
}
template <class A> Pipe<A, A> idPipe() { return purePipe<A, A>([](const A &a) { return a; }); }

// handlePipe: the Pipe around one native handle H, and the only place that wraps a csdr_* handle.  start runs create(&h), which may
// take more than one call (symSyncC); a throw from it destroys whatever handle it had made, once.  The handle then lives as long
// as the last holder of the resource (unPipe's closures, AddPipe), not until done, which has nothing left to do.  process gets
// the typed handle.
template <class H, class A, class B, class Create, class Destroy, class Process> Pipe<A, B> handlePipe(Create create, Destroy destroy, Process process)
{
    Pipe<A, B> p;
    p.start = [create, destroy]() {
        H *h = nullptr;
        try { create(&h); } catch (...) { if (h) destroy(h); throw; }
        return std::shared_ptr<void>(h, [destroy](void *q) { destroy(static_cast<H *>(q)); });
    };
    p.process = [process](void *r, const A &a) { return process(static_cast<H *>(r), a); };
    p.done = [](void *) {};
    return p;
}

// unPipe (Types.hs:109-115): `r <- creat; return (S.mapM (process r), dest r)`.  The stream side here is a push
// loop, so the transformer is the per-array function S.mapM would apply; `cleanup` is run once the stream has been
// folded (SoapySDR.hs:206, :282).
template <class A, class B> struct UnPiped {
    std::function<B(const A &)> process;
    std::function<void()> cleanup;
};
template <class A, class B> UnPiped<A, B> unPipe(Pipe<A, B> p)
{
    std::shared_ptr<void> r = p.start();
    UnPiped<A, B> u;
    u.process = [p, r](const A &a) { return p.process(r.get(), a); };
    u.cleanup = [p, r]() { p.done(r.get()); };
    return u;
}

// ---- Fold -------------------------------------------------------------------------------
template <class A> struct Fold {
    virtual ~Fold() = default;
    virtual void step(const A &a) = 0;
    virtual void done() = 0;
};

template <class A, class B> struct AddPipe : Fold<A> {
    Pipe<A, B> pipe; std::shared_ptr<Fold<B>> down; std::shared_ptr<void> r;
    AddPipe(Pipe<A, B> p, std::shared_ptr<Fold<B>> d) : pipe(std::move(p)), down(std::move(d)), r(pipe.start()) {}
    void step(const A &a) override { down->step(pipe.process(r.get(), a)); }
    void done() override { pipe.done(r.get()); down->done(); }
};
template <class A, class B> std::shared_ptr<Fold<A>> addPipe(Pipe<A, B> p, std::shared_ptr<Fold<B>> d)
{
    return std::make_shared<AddPipe<A, B>>(std::move(p), std::move(d));
}

template <class T> struct Compact : Fold<Array<T>> {
    size_t n; std::shared_ptr<Fold<Array<T>>> down; Array<T> buf;
    Compact(size_t n_, std::shared_ptr<Fold<Array<T>>> d) : n(n_), down(std::move(d)) {}
    void step(const Array<T> &a) override {
        buf.insert(buf.end(), a.begin(), a.end());
        if (buf.size() >= n) {                              // emit EXACTLY n, keep the rest (even if >= n)
            Array<T> head(buf.begin(), buf.begin() + n);
            buf.erase(buf.begin(), buf.begin() + n);
            down->step(head);
        }
    }
    void done() override { down->step(buf); buf.clear(); down->done(); }   // remainder pushed even when empty
};
template <class T> std::shared_ptr<Fold<Array<T>>> compact(size_t n, std::shared_ptr<Fold<Array<T>>> d)
{
    return std::make_shared<Compact<T>>(n, std::move(d));
}

template <class T> struct Distribute : Fold<std::vector<Array<T>>> {
    std::vector<std::shared_ptr<Fold<Array<T>>>> folds;
    explicit Distribute(std::vector<std::shared_ptr<Fold<Array<T>>>> f) : folds(std::move(f)) {}
    void step(const std::vector<Array<T>> &as) override { for (size_t k = 0; k < folds.size() && k < as.size(); k++) folds[k]->step(as[k]); }
    void done() override { for (auto &f : folds) f->done(); }
};

template <class T> Array<T> mix(const std::vector<Array<T>> &chans)
{
    Array<T> acc = chans.at(0);
    for (size_t k = 1; k < chans.size(); k++) {
        if (chans[k].size() < acc.size()) acc.resize(chans[k].size());       // zipWith truncates
        for (size_t i = 0; i < acc.size(); i++) acc[i] = acc[i] + chans[k][i];
    }
    return acc;
}

// takeNArr as a push-side limiter: returns false once the stream is finished
struct TakeN {
    size_t n, seen = 0;
    explicit TakeN(size_t n_) : n(n_) {}
    template <class T> bool feed(Array<T> &a) {
        if (seen == n) return false;
        if (n - seen < a.size()) a.resize(n - seen);
        seen += a.size();
        return true;
    }
};

template <class T> struct FileSink : Fold<Array<T>> {
    FILE *f;
    explicit FileSink(const std::string &path) : f(std::fopen(path.c_str(), "wb")) { if (!f) throw std::runtime_error("cannot open " + path); }
    ~FileSink() override { if (f) std::fclose(f); }
    void step(const Array<T> &a) override { if (!a.empty() && std::fwrite(a.data(), sizeof(T), a.size(), f) != a.size()) throw std::runtime_error("short write"); }
    void done() override { if (f) { std::fclose(f); f = nullptr; } }
};

// audioFileSink fmt sr sn nch fp (Sink.hs:41-74): libsndfile float, big-endian, fp + ".au" / ".wav".  AU: 24-byte
// header (".snd", 24, data bytes, 6 = IEEE float, rate, channels).  WAV: libsndfile writes RIFX with a time-stamped
// PEAK chunk (not reproducible); this writer emits RIFX + fmt(tag 3) + fact + data.  Unverified against libsndfile.
struct AudioFileSink : Fold<Array<float>> {
    FILE *f = nullptr; bool au; uint32_t sr, nch; uint64_t nbytes = 0; std::string path;
    static void be32(unsigned char *p, uint32_t v) { p[0] = v >> 24; p[1] = v >> 16; p[2] = v >> 8; p[3] = v; }
    static void be16(unsigned char *p, uint16_t v) { p[0] = v >> 8; p[1] = v & 255; }
    AudioFileSink(const std::string &fmt, uint32_t sr_, uint32_t nch_, const std::string &fp)
        : au(fmt == "AU" || fmt == "au"), sr(sr_), nch(nch_), path(fp + ((fmt == "AU" || fmt == "au") ? ".au" : ".wav"))
    {
        f = std::fopen(path.c_str(), "wb");
        if (!f) throw std::runtime_error("cannot open " + path);
        header(au ? 0xffffffffu : 0u);
    }
    ~AudioFileSink() override { if (f) std::fclose(f); }
    void header(uint32_t n)
    {
        unsigned char h[56];
        std::fseek(f, 0, SEEK_SET);
        if (au) {
            std::memcpy(h, ".snd", 4); be32(h + 4, 24); be32(h + 8, n); be32(h + 12, 6); be32(h + 16, sr); be32(h + 20, nch);
            std::fwrite(h, 1, 24, f);
        } else {
            std::memcpy(h, "RIFX", 4); be32(h + 4, 4 + 24 + 12 + 8 + n); std::memcpy(h + 8, "WAVE", 4);
            std::memcpy(h + 12, "fmt ", 4); be32(h + 16, 16); be16(h + 20, 3); be16(h + 22, (uint16_t)nch); be32(h + 24, sr);
            be32(h + 28, sr * 4 * nch); be16(h + 32, (uint16_t)(4 * nch)); be16(h + 34, 32);
            std::memcpy(h + 36, "fact", 4); be32(h + 40, 4); be32(h + 44, n / (4 * nch));
            std::memcpy(h + 48, "data", 4); be32(h + 52, n);
            std::fwrite(h, 1, 56, f);
        }
    }
    void step(const Array<float> &a) override
    {
        std::vector<unsigned char> b(a.size() * 4);
        for (size_t i = 0; i < a.size(); i++) { uint32_t u; std::memcpy(&u, &a[i], 4); be32(b.data() + 4 * i, u); }
        if (!b.empty() && std::fwrite(b.data(), 1, b.size(), f) != b.size()) throw std::runtime_error("short write");
        nbytes += b.size();
    }
    void done() override { if (f) { header((uint32_t)nbytes); std::fclose(f); f = nullptr; } }
};

// ---- front-end Pipes: resampler r as (Liquid.chs:115-117), mixDown / mixUp f (Liquid.chs:805-809) ----
inline Pipe<Array<cf32>, Array<cf32>> resampler(float r, float as_db, uint32_t max_in)
{
    return handlePipe<csdr_resamp, Array<cf32>, Array<cf32>>(
        [=](csdr_resamp **h) { check(csdr_resamp_create(r, as_db, max_in, h)); }, csdr_resamp_destroy,
        [](csdr_resamp *h, const Array<cf32> &a) {
            Array<cf32> y(csdr_resamp_max_out(h, (uint32_t)a.size()));          // 2*ceil(r*nx), Liquid.chs:81
            uint32_t n = 0;
            check(csdr_resamp_process(h, reinterpret_cast<const float *>(a.data()), (uint32_t)a.size(), reinterpret_cast<float *>(y.data()), &n));
            y.resize(n);                                                         // shrinkToFit, Liquid.chs:98
            return y;
        });
}
inline Pipe<Array<cf32>, Array<cf32>> ncoMixer(float f, bool up, uint32_t max_in)
{
    return handlePipe<csdr_nco, Array<cf32>, Array<cf32>>(
        [=](csdr_nco **h) { check(csdr_nco_create(f, max_in, h)); }, csdr_nco_destroy,
        [up](csdr_nco *h, const Array<cf32> &a) {
            Array<cf32> y(a.size());
            if (!a.empty())
                check((up ? csdr_nco_mix_up : csdr_nco_mix_down)(h, reinterpret_cast<const float *>(a.data()), (uint32_t)a.size(), reinterpret_cast<float *>(y.data())));
            return y;
        });
}
inline Pipe<Array<cf32>, Array<cf32>> mixDown(float f, uint32_t max_in) { return ncoMixer(f, false, max_in); }
inline Pipe<Array<cf32>, Array<cf32>> mixUp(float f, uint32_t max_in) { return ncoMixer(f, true, max_in); }

// ---- realToComplex / complexToReal (Liquid.chs:536-537, 545-546): firhilbf_create 5 60 as a 2:1 decimator / 1:2 interpolator;
// max_in in complex samples.  An odd-length float array loses its last float (firhilbDecim's `length div 2`) ----
inline Pipe<Array<float>, Array<cf32>> realToComplex(uint32_t max_in, uint32_t m = 5, float as_db = 60.0f)
{
    return handlePipe<csdr_firhilb, Array<float>, Array<cf32>>(
        [=](csdr_firhilb **h) { check(csdr_firhilb_create(m, as_db, max_in, h)); }, csdr_firhilb_destroy,
        [](csdr_firhilb *h, const Array<float> &a) {
            Array<cf32> y(a.size() / 2);
            check(csdr_firhilb_decim(h, a.data(), (uint32_t)y.size(), reinterpret_cast<float *>(y.data())));
            return y;
        });
}
inline Pipe<Array<cf32>, Array<float>> complexToReal(uint32_t max_in, uint32_t m = 5, float as_db = 60.0f)
{
    return handlePipe<csdr_firhilb, Array<cf32>, Array<float>>(
        [=](csdr_firhilb **h) { check(csdr_firhilb_create(m, as_db, max_in, h)); }, csdr_firhilb_destroy,
        [](csdr_firhilb *h, const Array<cf32> &a) {
            Array<float> y(2 * a.size());
            check(csdr_firhilb_interp(h, reinterpret_cast<const float *>(a.data()), (uint32_t)a.size(), y.data()));
            return y;
        });
}

// ---- openAudioFile / readFromAudioFile (Source.chs:273-307) without libsndfile: a hand-written reader, as AudioFileSink is a
// hand-written writer.  RIFF / RIFX WAV with fmt tag 1 (PCM 8 / 16 / 24 / 32), 3 (IEEE float 32 / 64) or 0xFFFE (the tag is the
// sub-format's first two bytes), other chunks skipped; .snd AU with encoding 2, 3, 4, 5 (PCM 8 / 16 / 24 / 32), 6, 7 (float
// 32 / 64).  read() is libsndfile's float read: PCM16 / 32768, PCM24 / 8388608, PCM32 / 2147483648, WAV's unsigned 8 bit
// (v - 128) / 128, AU's signed 8 bit / 128.  A data size of 0 or 0xffffffff means "to the end of the file" ----
struct SourceError : std::runtime_error { using std::runtime_error::runtime_error; };
struct AudioFile {
    enum Kind { U8, INT, FLOAT };
    FILE *f = nullptr; uint32_t channels = 0, rate = 0, width = 0; Kind kind = INT; bool big = false; uint64_t left = 0;
    ~AudioFile() { if (f) std::fclose(f); }
    static uint32_t u32(const unsigned char *p, bool be) { return be ? (uint32_t)p[0] << 24 | p[1] << 16 | p[2] << 8 | p[3] : (uint32_t)p[3] << 24 | p[2] << 16 | p[1] << 8 | p[0]; }
    static uint32_t u16(const unsigned char *p, bool be) { return be ? p[0] << 8 | p[1] : p[1] << 8 | p[0]; }
    // the AudioFile of `path`, or null when the header is neither WAV nor AU (the caller then reads raw CF32)
    static std::unique_ptr<AudioFile> open(const std::string &path)
    {
        FILE *f = std::fopen(path.c_str(), "rb");
        if (!f) throw SourceError("Unable to open source: " + path);
        std::unique_ptr<AudioFile> a(new AudioFile());
        a->f = f;
        std::fseek(f, 0, SEEK_END);
        const uint64_t size = (uint64_t)std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        unsigned char head[12];
        const size_t got = std::fread(head, 1, 12, f);
        auto fail = [&](const std::string &why) -> std::unique_ptr<AudioFile> { throw SourceError("Unable to open source: " + path + ": " + why); };
        if (got >= 12 && (!std::memcmp(head, "RIFF", 4) || !std::memcmp(head, "RIFX", 4)) && !std::memcmp(head + 8, "WAVE", 4)) {
            const bool be = head[3] == 'X';
            bool have_fmt = false; uint32_t tag = 0, bits = 0;
            for (uint64_t pos = 12; pos + 8 <= size;) {
                unsigned char ch[8], b[40];
                std::fseek(f, (long)pos, SEEK_SET);
                if (std::fread(ch, 1, 8, f) != 8) break;
                const uint32_t csz = u32(ch + 4, be);
                if (!std::memcmp(ch, "fmt ", 4)) {
                    const size_t nb = std::fread(b, 1, csz < 40 ? csz : 40, f);
                    if (nb < 16) return fail("short fmt chunk");
                    tag = u16(b, be); a->channels = u16(b + 2, be); a->rate = u32(b + 4, be); bits = u16(b + 14, be);
                    if (tag == 0xFFFE && nb >= 26) tag = u16(b + 24, be);
                    have_fmt = true;
                } else if (!std::memcmp(ch, "data", 4)) {
                    if (!have_fmt) return fail("data chunk before fmt");
                    if (!((tag == 1 && (bits == 8 || bits == 16 || bits == 24 || bits == 32)) || (tag == 3 && (bits == 32 || bits == 64))))
                        return fail("WAV format tag " + std::to_string(tag) + " with " + std::to_string(bits) + " bits is not supported");
                    const uint64_t avail = size - (pos + 8);
                    const uint64_t nbytes = (csz == 0 || csz == 0xffffffffu) ? avail : (csz < avail ? csz : avail);
                    a->kind = tag == 3 ? FLOAT : (bits == 8 ? U8 : INT); a->width = bits / 8; a->big = be;
                    a->left = nbytes / a->width * a->width;
                    return a;                                      // the file position is the first sample
                }
                pos += 8 + (uint64_t)csz + (csz & 1);
            }
            return fail("WAV without a data chunk");
        }
        if (got >= 4 && !std::memcmp(head, ".snd", 4)) {
            unsigned char b[24];
            std::fseek(f, 0, SEEK_SET);
            if (std::fread(b, 1, 24, f) != 24) return fail("short AU header");
            const uint32_t off = u32(b + 4, true), dsz = u32(b + 8, true), enc = u32(b + 12, true);
            a->rate = u32(b + 16, true); a->channels = u32(b + 20, true);
            if (enc < 2 || enc > 7 || off < 24 || off > size) return fail("AU encoding " + std::to_string(enc) + " is not supported");
            static const uint32_t widths[8] = {0, 0, 1, 2, 3, 4, 4, 8};
            a->kind = enc >= 6 ? FLOAT : INT; a->width = widths[enc]; a->big = true;
            const uint64_t avail = size - off;
            a->left = ((dsz == 0 || dsz == 0xffffffffu) ? avail : (dsz < avail ? dsz : avail)) / a->width * a->width;
            std::fseek(f, (long)off, SEEK_SET);
            return a;
        }
        return nullptr;
    }
    // hGetBuffer h n: up to n floats (fewer at the end of the data, none after it)
    Array<float> read(size_t n)
    {
        uint64_t want = (uint64_t)n * width;
        if (want > left) want = left;
        std::vector<unsigned char> b(want);
        size_t gotb = want ? std::fread(b.data(), 1, want, f) : 0;
        gotb = gotb / width * width;
        left -= gotb;
        Array<float> y(gotb / width);
        for (size_t i = 0; i < y.size(); i++) {
            const unsigned char *p = b.data() + i * width;
            unsigned char q[8];
            for (uint32_t j = 0; j < width; j++) q[j] = big ? p[width - 1 - j] : p[j];       // little-endian now
            if (kind == FLOAT) {
                if (width == 4) std::memcpy(&y[i], q, 4);
                else { double d; std::memcpy(&d, q, 8); y[i] = (float)d; }
            } else if (kind == U8) y[i] = (float)((int)q[0] - 128) / 128.0f;
            else {
                uint32_t u = 0;
                for (uint32_t j = 0; j < width; j++) u |= (uint32_t)q[j] << (8 * (j + 4 - width));   // left-aligned in 32 bits
                const int32_t v = (int32_t)u >> (8 * (4 - width));                                      // sign-extended
                y[i] = (float)v * (1.0f / (float)(1ull << (8 * width - 1)));
            }
        }
        return y;
    }
};

// initFileSource (SoapySDR.hs:172-179): every file is tried as an audio file first and read as raw CF32 otherwise.  An audio
// source must be mono ("Unable to open source", no fall-back to raw) and yields, per `chunk` floats read,
// mixUp (2 pi 0.5) . realToComplex of them: chunk / 2 samples.  DEVIATION: the reference drops the last float of every chunk when
// chunk is odd while liquid's windows run on; an odd chunk is refused for an audio source instead.  A last, short chunk with an
// odd count drops its last float.
struct FileSource {
    FILE *f = nullptr; std::unique_ptr<AudioFile> audio; size_t chunk;
    UnPiped<Array<float>, Array<cf32>> front; bool have_front = false;
    FileSource(const std::string &path, size_t chunk_) : chunk(chunk_)
    {
        audio = AudioFile::open(path);
        if (!audio) {
            f = std::fopen(path.c_str(), "rb");
            if (!f) throw SourceError("Unable to open source: " + path);
            return;
        }
        if (audio->channels != 1)
            throw SourceError("Unable to open source: " + path + " has " + std::to_string(audio->channels) + " channels, an audio source must be mono");
        if (chunk % 2)
            throw SourceError("Unable to open source: " + path + " is an audio file and needs an even --chunksize (got " + std::to_string(chunk) + ")");
        const float fm = (float)(2.0 * 3.14159265358979323846 * 0.5);          // the Haskell Float 2 * pi * 0.5
        front = unPipe(compose(mixUp(fm, (uint32_t)(chunk / 2)), realToComplex((uint32_t)(chunk / 2))));
        have_front = true;
    }
    ~FileSource() { if (f) std::fclose(f); }
    // the next array; false at the end of the file
    bool next(Array<cf32> &a)
    {
        if (audio) {
            const Array<float> x = audio->read(chunk);
            if (x.empty()) return false;
            a = front.process(x);
            return true;
        }
        a.resize(chunk);
        const size_t got = std::fread(a.data(), sizeof(cf32), chunk, f);
        a.resize(got);
        return got != 0;
    }
    void close() { if (have_front) { front.cleanup(); have_front = false; } }
};

// ---- DeFMS's per-chunk Pipes (SoapySDR.hs:261-264): automaticGainControl tres (Liquid.chs:727-728), fmDemodulator kf
// (Liquid.chs:333-334), stereoFMDecoder quadRate decim (Liquid.chs:1069-1078; interleaved L, R out) ----
inline Pipe<Array<cf32>, Array<cf32>> agcPipe(float tres, uint32_t max_in)
{
    return handlePipe<csdr_agc, Array<cf32>, Array<cf32>>(
        [=](csdr_agc **h) { check(csdr_agc_create(tres, 1, max_in, h)); }, csdr_agc_destroy,
        [](csdr_agc *h, const Array<cf32> &a) {
            Array<cf32> y(a.size());
            if (!a.empty())
                check(csdr_agc_process(h, reinterpret_cast<const float *>(a.data()), (uint32_t)a.size(), reinterpret_cast<float *>(y.data())));
            return y;
        });
}
inline Pipe<Array<cf32>, Array<float>> freqdemPipe(float kf, uint32_t max_in)
{
    return handlePipe<csdr_freqdem, Array<cf32>, Array<float>>(
        [=](csdr_freqdem **h) { check(csdr_freqdem_create(kf, 1, max_in, h)); }, csdr_freqdem_destroy,
        [](csdr_freqdem *h, const Array<cf32> &a) {
            Array<float> m(a.size());
            if (!a.empty()) check(csdr_freqdem_process(h, reinterpret_cast<const float *>(a.data()), (uint32_t)a.size(), m.data()));
            return m;
        });
}
inline Pipe<Array<float>, Array<float>> fmStereoPipe(float quad_rate, uint32_t decim, uint32_t max_in)
{
    return handlePipe<csdr_fmstereo, Array<float>, Array<float>>(
        [=](csdr_fmstereo **h) { check(csdr_fmstereo_create(quad_rate, decim, 1, max_in, h)); }, csdr_fmstereo_destroy,
        [decim](csdr_fmstereo *h, const Array<float> &a) {
            Array<float> y(2 * (a.size() / decim));
            uint32_t n = 0;
            if (!a.empty()) check(csdr_fmstereo_process(h, a.data(), (uint32_t)a.size(), y.data(), &n));
            y.resize(n);
            return y;
        });
}

// ---- Pipes on the channel rows of one chunk: one handle with one stream (or filter state) per row for the whole run ----
// The rows go to the C ABI as one flat [nchan][n] array and come back cut into rows.  The shape rule of every such Pipe: a
// chunk whose row count is not nchan, or whose first row is empty (nx = 0 -> [empty]), passes through as rows.size() empty arrays
// without a call.  Rows of unequal length throw a std::runtime_error that names the pipe, before anything is copied (the
// copy used to be sized by rows[0] alone: a longer row wrote past the end of the heap buffer, a shorter one was zero-padded).
template <class T> using Rows = std::vector<Array<T>>;

// rows -> flat [nchan][n] with n = rows[0].size(); empty = "pass the chunk through" (the shape rule)
template <class T> Array<T> flattenRows(const Rows<T> &rows, uint32_t nchan, const char *pipe)
{
    if (rows.size() != nchan || rows.empty() || rows[0].empty()) return {};
    const size_t n = rows[0].size();
    for (const Array<T> &r : rows)
        if (r.size() != n) throw std::runtime_error(std::string(pipe) + ": the rows of one chunk must have one length");
    Array<T> flat(nchan * n);
    for (uint32_t c = 0; c < nchan; c++) std::copy(rows[c].begin(), rows[c].end(), flat.begin() + c * n);
    return flat;
}
// flat, rows `stride` apart -> row c = its first counts[c] elements; one count for every row is the special case
template <class T> Rows<T> splitRows(const Array<T> &flat, uint32_t nchan, size_t stride, const std::vector<uint32_t> &counts)
{
    Rows<T> out;
    for (uint32_t c = 0; c < nchan; c++) out.emplace_back(flat.begin() + c * stride, flat.begin() + c * stride + counts[c]);
    return out;
}
template <class T> Rows<T> splitRows(const Array<T> &flat, uint32_t nchan, size_t stride, size_t count)
{
    return splitRows(flat, nchan, stride, std::vector<uint32_t>(nchan, (uint32_t)count));
}
// handlePipe on rows: call(h, flat, n) runs the ABI on the flat [nchan][n] input and returns the output rows
template <class H, class A, class B, class Create, class Destroy, class Call>
Pipe<Rows<A>, Rows<B>> rowPipe(const char *pipe, uint32_t nchan, Create create, Destroy destroy, Call call)
{
    return handlePipe<H, Rows<A>, Rows<B>>(create, destroy, [=](H *h, const Rows<A> &rows) {
        const Array<A> x = flattenRows(rows, nchan, pipe);
        return x.empty() ? Rows<B>(rows.size()) : call(h, x, (uint32_t)(x.size() / nchan));
    });
}

// ---- symSyncR k m beta M (Liquid.chs:244-282; set_lf_bw 0.05, set_output_rate 2): row c of the output holds that stream's
// ny[c] samples ----
inline Pipe<Rows<float>, Rows<float>> symSyncR(uint32_t k, uint32_t m, float beta, uint32_t M, uint32_t nchan, uint32_t max_in)
{
    return rowPipe<csdr_symsync, float, float>(
        "symSyncR", nchan, [=](csdr_symsync **h) { check(csdr_symsync_create(k, m, beta, M, 0.05f, 2, nchan, max_in, h)); }, csdr_symsync_destroy,
        [nchan](csdr_symsync *h, const Array<float> &x, uint32_t n) {
            Array<float> y(x.size());
            std::vector<uint32_t> ny(nchan);
            check(csdr_symsync_process(h, x.data(), n, y.data(), ny.data()));
            return splitRows(y, nchan, n, ny);
        });
}

// ---- symSyncC m k (Liquid.chs:177-242; symsync_crcf_create_rnyquist(ARKAISER, k, m, 0.5, 32), lf_bw 0.01 and output rate 1 at
// symsync_create's defaults) on CF32 rows, e.g. firpfbchChannelizer's: row c of the output holds that stream's ny[c] symbols ----
inline Pipe<Rows<cf32>, Rows<cf32>> symSyncC(uint32_t m, uint32_t k, uint32_t nchan, uint32_t max_in)
{
    return rowPipe<csdr_symsync, cf32, cf32>(
        "symSyncC", nchan,
        [=](csdr_symsync **h) {
            check(csdr_symsync_create(k, m, 0.0f, 32, 0.01f, 1, nchan, max_in, h));
            check(csdr_symsync_set_rnyquist(*h, CSDR_FIRFILT_ARKAISER, 0.5f));
        },
        csdr_symsync_destroy,
        [nchan](csdr_symsync *h, const Array<cf32> &x, uint32_t n) {
            Array<cf32> y(x.size());
            std::vector<uint32_t> ny(nchan);
            check(csdr_symsync_process_c(h, reinterpret_cast<const float *>(x.data()), n, reinterpret_cast<float *>(y.data()), ny.data()));
            return splitRows(y, nchan, n, ny);
        });
}

// ---- pskTracker: power normaliser, carrier PLL, T/2 equaliser and BPSK / QPSK decisions on CF32 rows of their own
// lengths, as symSyncC yields them (zero-padded to the longest, with the counts beside them); row c of the output holds that row's
// soft symbols.  symTracker m k (Liquid.chs:119-175; symtrack_cccf_create(RRC, k, m, 0.25, BPSK)) is the composition: csdr_symsync
// with npfb 16, lf_bw 0.01, output rate 2 and the RRC 0.25 banks, then PskTracker(bits 1, sps 2, phase 0, eq_len 9, constant modulus) ----
inline Pipe<Rows<cf32>, Rows<cf32>> PskTracker(uint32_t bits, uint32_t sps, uint32_t phase, uint32_t eq_len, uint32_t eq_mode, uint32_t nchan,
                                               uint32_t max_in)
{
    return handlePipe<csdr_psktrack, Rows<cf32>, Rows<cf32>>(
        [=](csdr_psktrack **h) {
            check(csdr_psktrack_new(bits, sps, phase, eq_len, CSDR_PSKTRACK_EQ_MU, eq_mode, CSDR_PSKTRACK_EQ_DELAY, CSDR_PSKTRACK_PLL_BW,
                                    CSDR_PSKTRACK_AGC_BW, nchan, max_in, h));
        },
        csdr_psktrack_destroy,
        [nchan](csdr_psktrack *h, const Rows<cf32> &rows) {
            if (rows.size() != nchan) return Rows<cf32>(rows.size());
            std::vector<uint32_t> nx(nchan), ny(nchan);
            size_t n = 0;
            for (uint32_t c = 0; c < nchan; c++) { nx[c] = (uint32_t)rows[c].size(); n = std::max(n, rows[c].size()); }
            if (!n) return Rows<cf32>(rows.size());
            Array<cf32> x(nchan * n), y(nchan * n);
            for (uint32_t c = 0; c < nchan; c++) std::copy(rows[c].begin(), rows[c].end(), x.begin() + c * n);
            check(csdr_psktrack_process(h, reinterpret_cast<const float *>(x.data()), (uint32_t)n, nx.data(), reinterpret_cast<float *>(y.data()),
                                        nullptr, ny.data()));
            return splitRows(y, nchan, n, ny);
        });
}
inline Pipe<Rows<cf32>, Rows<cf32>> symTracker(uint32_t m, uint32_t k, uint32_t nchan, uint32_t max_in)
{
    auto sync = rowPipe<csdr_symsync, cf32, cf32>(
        "symTracker", nchan,
        [=](csdr_symsync **h) {
            check(csdr_symsync_create(k, m, 0.0f, 16, 0.01f, 2, nchan, max_in, h));
            check(csdr_symsync_set_rnyquist(*h, CSDR_FIRFILT_RRC, 0.25f));
        },
        csdr_symsync_destroy,
        [nchan](csdr_symsync *h, const Array<cf32> &x, uint32_t n) {
            Array<cf32> y(x.size());
            std::vector<uint32_t> ny(nchan);
            check(csdr_symsync_process_c(h, reinterpret_cast<const float *>(x.data()), n, reinterpret_cast<float *>(y.data()), ny.data()));
            return splitRows(y, nchan, n, ny);
        });
    return compose(PskTracker(1, 2, 0, 9, CSDR_PSKTRACK_EQ_CM, nchan, max_in), sync);
}

// ---- fskDemodulator m k bw (Liquid.chs:336-382): row c of the output holds the n div k symbols of row c, the n mod k samples
// left over are dropped (:367-376).  gmskDemodulator m k bw (Liquid.chs:384-429; the reference's argument order, gmskdem_create
// takes k m bw): the n / k bits of row c; a row length that is no multiple of k throws, as :421 does ----
namespace detail {
template <class H, class Create, class Destroy>
Pipe<Rows<cf32>, Rows<uint32_t>> symbolRows(const char *pipe, uint32_t k, uint32_t nchan, Create create, Destroy destroy,
                                            int (*process)(H *, const float *, uint32_t, uint32_t *, float *, uint32_t *))
{
    return rowPipe<H, cf32, uint32_t>(pipe, nchan, create, destroy, [=](H *h, const Array<cf32> &x, uint32_t n) {
        const size_t ns = n / k;
        Array<uint32_t> sym(nchan * ns);
        uint32_t n_out = 0;
        check(process(h, reinterpret_cast<const float *>(x.data()), n, sym.data(), nullptr, &n_out));
        return splitRows(sym, nchan, ns, ns);
    });
}
}  // namespace detail
inline Pipe<Rows<cf32>, Rows<uint32_t>> FskDemodulator(uint32_t m, uint32_t k, float bw, uint32_t nchan, uint32_t max_in)
{
    return detail::symbolRows<csdr_fskdem>(
        "FskDemodulator", k, nchan, [=](csdr_fskdem **h) { check(csdr_fskdem_create(m, k, bw, nchan, max_in, h)); }, csdr_fskdem_destroy,
        csdr_fskdem_process);
}
inline Pipe<Rows<cf32>, Rows<uint32_t>> GmskDemodulator(uint32_t m, uint32_t k, float bw, uint32_t nchan, uint32_t max_in)
{
    return detail::symbolRows<csdr_gmskdem>(
        "GmskDemodulator", k, nchan, [=](csdr_gmskdem **h) { check(csdr_gmskdem_create(k, m, bw, nchan, max_in, h)); }, csdr_gmskdem_destroy,
        csdr_gmskdem_process);
}

// ---- firFilterCKaiser n fc as mu / firFilterC f / firFilterR f (Liquid.chs:868-916, 955-957): one csdr_firfilt handle with one
// filter state per row; the liquid object f is its taps and scale here.  iirCFilter n fc f0 ap as (Liquid.chs:594-608) and the
// caller's own second-order sections: one csdr_iirsos handle with one state per row and section; a liquid iirfilt object is its
// sections here (b, a: [S][3] each, row-major).  Both give n samples out for n in ----
namespace detail {
template <class H, class T, class Create, class Destroy>
Pipe<Rows<T>, Rows<T>> filterRows(const char *pipe, uint32_t nchan, Create create, Destroy destroy, int (*process)(H *, const float *, uint32_t, float *))
{
    return rowPipe<H, T, T>(pipe, nchan, create, destroy, [=](H *h, const Array<T> &x, uint32_t n) {
        Array<T> y(x.size());
        check(process(h, reinterpret_cast<const float *>(x.data()), n, reinterpret_cast<float *>(y.data())));
        return splitRows(y, nchan, n, n);
    });
}
template <class T> Pipe<Rows<T>, Rows<T>> firFilterTaps(const char *pipe, const Array<float> &taps, float scale, uint32_t nchan, uint32_t max_in)
{
    return filterRows<csdr_firfilt, T>(pipe, nchan, [=](csdr_firfilt **h) {
        check(csdr_firfilt_create_taps(taps.data(), (uint32_t)taps.size(), scale, std::is_same<T, cf32>::value, nchan, max_in, h));
    }, csdr_firfilt_destroy, csdr_firfilt_process);
}
}  // namespace detail
inline Pipe<Rows<cf32>, Rows<cf32>> FirFilterC(const Array<float> &taps, float scale, uint32_t nchan, uint32_t max_in)
{
    return detail::firFilterTaps<cf32>("FirFilterC", taps, scale, nchan, max_in);
}
inline Pipe<Rows<float>, Rows<float>> FirFilterR(const Array<float> &taps, float scale, uint32_t nchan, uint32_t max_in)
{
    return detail::firFilterTaps<float>("FirFilterR", taps, scale, nchan, max_in);
}
inline Pipe<Rows<cf32>, Rows<cf32>> FirFilterCKaiser(uint32_t n, float fc, float as_db, float mu, uint32_t nchan, uint32_t max_in)
{
    return detail::filterRows<csdr_firfilt, cf32>("FirFilterCKaiser", nchan, [=](csdr_firfilt **h) {
        check(csdr_firfilt_create_kaiser(n, fc, as_db, mu, 1, nchan, max_in, h));
    }, csdr_firfilt_destroy, csdr_firfilt_process);
}

// ---- firFilterRNyquist k m beta mu (Liquid.chs:935-953: LIQUID_FIRFILT_GMSKRX and the scale 1 / k are hard-coded there):
// FirFilterR on the taps of csdr_firdes_gmskrx(k, m, beta); mu != 0 is refused ----
inline Pipe<Rows<float>, Rows<float>> FirFilterRNyquist(uint32_t k, uint32_t m, float beta, float mu, uint32_t nchan, uint32_t max_in)
{
    if (mu != 0.f) throw std::runtime_error("FirFilterRNyquist: mu != 0 is not supported");
    Array<float> taps(2 * (size_t)k * m + 1);
    check(csdr_firdes_gmskrx(k, m, beta, taps.data()));
    return detail::firFilterTaps<float>("FirFilterRNyquist", taps, 1.0f / (float)k, nchan, max_in);
}

inline Pipe<Rows<cf32>, Rows<cf32>> IirCFilter(uint32_t n, float fc, float f0, float ap, float as_db, uint32_t nchan, uint32_t max_in)
{
    return detail::filterRows<csdr_iirsos, cf32>("IirCFilter", nchan, [=](csdr_iirsos **h) {
        check(csdr_iirsos_create_prototype(n, fc, f0, ap, as_db, 1, nchan, max_in, h));
    }, csdr_iirsos_destroy, csdr_iirsos_process);
}
template <class T> Pipe<Rows<T>, Rows<T>> IirFilterSOS(const Array<float> &b, const Array<float> &a, uint32_t nchan, uint32_t max_in)
{
    return detail::filterRows<csdr_iirsos, T>("IirFilterSOS", nchan, [=](csdr_iirsos **h) {
        if (b.size() != a.size() || b.size() % 3) throw std::runtime_error("IirFilterSOS: b and a must hold 3 floats per section each");
        check(csdr_iirsos_create_sos(b.data(), a.data(), (uint32_t)(b.size() / 3), std::is_same<T, cf32>::value, nchan, max_in, h));
    }, csdr_iirsos_destroy, csdr_iirsos_process);
}

// ---- the fused chain as a Pipe (replaces mix . mux (replicate nch demod) . firpfbchChannelizer nc) ----
struct ChainOpts {
    uint32_t channels = 1; bool dc_block = true; float agc = 0.f; bool fm = false; bool am = false; bool wbfm = false; uint32_t decim = 4; float deemph_fc = 0.025f; float kf = 0.3f; bool mix = false;
    uint32_t max_frames = 4096; uint32_t flags = CSDR_FLAG_QUIET;
    // channel shard of a multi-GPU run (one process per GPU): this process owns the channels rank, rank + world, ... (interleaved
    // ownership); with mix the partial sums meet in ONE all-reduce per chunk (csdr_chain_process_mix over `comm`)
    uint32_t world = 1, rank = 0; csdr_comm *comm = nullptr; int device = -1;       // device: HIP ordinal of this process's GPU (-1 = current)
    uint32_t owned() const { return world > 1 ? channels / world : channels; }
    uint32_t channel_of(uint32_t row) const { return world > 1 ? rank + world * row : row; }       // 0-based channel of output row `row`
};

// csdr_comm bootstrap through a file (RCCL's unique id is 128 opaque bytes that rank 0 makes and every rank needs): rank 0 writes
// `path` atomically, the others wait for it.  device -1 = current.
// The file is  "CSDRID01" | uint64 nonce | id : a waiting rank accepts it only when the nonce is its own run's, so the id a crashed
// earlier run left behind under the same path is never taken for this run's (ranks with different ids would block in
// ncclCommInitRank for ever).  nonce 0 = the launcher's pid (getppid(): the ranks of one run are children of one launcher); pass an
// explicit one (soapy_sdr_file --id-nonce N, a launcher pid or a timestamp) when the ranks do not share a parent.  Rank 0 removes
// the file once csdr_comm_create has returned -- that call is collective, so every rank has read the id by then.
inline uint64_t commRunNonce(uint64_t nonce) { return nonce ? nonce : (uint64_t)getppid(); }
inline bool commReadIdFile(const std::string &path, uint64_t nonce, unsigned char *id)
{
    unsigned char rec[16 + CSDR_COMM_ID_BYTES];
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    const size_t got = std::fread(rec, 1, sizeof rec, f);
    std::fclose(f);
    uint64_t have = 0;
    if (got != sizeof rec || std::memcmp(rec, "CSDRID01", 8) != 0) return false;
    std::memcpy(&have, rec + 8, 8);
    if (have != nonce) return false;                       // another run's id (stale file): keep waiting for ours
    std::memcpy(id, rec + 16, CSDR_COMM_ID_BYTES);
    return true;
}
inline void commWriteIdFile(const std::string &path, uint64_t nonce, const unsigned char *id)
{
    unsigned char rec[16 + CSDR_COMM_ID_BYTES];
    std::memcpy(rec, "CSDRID01", 8);
    std::memcpy(rec + 8, &nonce, 8);
    std::memcpy(rec + 16, id, CSDR_COMM_ID_BYTES);
    std::remove(path.c_str());                             // a stale id must not be readable while ours is being written
    const std::string tmp = path + ".tmp";
    FILE *f = std::fopen(tmp.c_str(), "wb");
    const bool ok = f && std::fwrite(rec, 1, sizeof rec, f) == sizeof rec;
    if (f) std::fclose(f);
    if (!ok) throw std::runtime_error("cannot write " + tmp);
    if (std::rename(tmp.c_str(), path.c_str()) != 0) throw std::runtime_error("cannot rename " + tmp);
}
inline csdr_comm *commFromIdFile(const std::string &path, int rank, int world, int device = -1, uint64_t nonce = 0)
{
    unsigned char id[CSDR_COMM_ID_BYTES];
    nonce = commRunNonce(nonce);
    if (rank == 0) {
        check(csdr_comm_unique_id(id));
        commWriteIdFile(path, nonce, id);
    } else {
        for (int tries = 0; !commReadIdFile(path, nonce, id); tries++) {
            if (tries > 6000) throw std::runtime_error("no communicator id of this run (nonce " + std::to_string(nonce) + ") in " + path + " after 60 s");
            struct timespec ts = {0, 10 * 1000 * 1000};
            nanosleep(&ts, nullptr);
        }
    }
    csdr_comm *c = nullptr;
    const int rc = csdr_comm_create(rank, world, id, device, &c);
    if (rank == 0) std::remove(path.c_str());              // every rank has joined (or the create failed): the id is spent
    check(rc);
    return c;
}

// ---- the 2x-oversampled firpfbchChannelizer (liquid's firpfbch2_crcf analyzer, which the reference does not import): M rows at
// 2 / M of the input rate, Kaiser prototype of semi-length m, attenuation as_db and cutoff fc (0: 1 / M); a chunk has to be a
// whole number of frames of M / 2 samples; an empty chunk yields [empty], as firpfbchChannelizer's ----
inline Pipe<Array<cf32>, std::vector<Array<cf32>>> Firpfbch2Channelizer(uint32_t M, uint32_t m, float as_db, float fc, uint32_t max_frames)
{
    return handlePipe<csdr_pfbch2, Array<cf32>, std::vector<Array<cf32>>>(
        [=](csdr_pfbch2 **h) { check(csdr_pfbch2_open_kaiser(M, m, as_db, fc, max_frames, h)); }, csdr_pfbch2_destroy,
        [M](csdr_pfbch2 *h, const Array<cf32> &a) {
            if (a.empty()) return std::vector<Array<cf32>>{Array<cf32>{}};
            Array<cf32> flat((size_t)2 * a.size());                          // [M][a.size() / (M / 2)]
            uint32_t frames = 0;
            check(csdr_pfbch2_process(h, reinterpret_cast<const float *>(a.data()), (uint32_t)a.size(), reinterpret_cast<float *>(flat.data()), &frames));
            std::vector<Array<cf32>> outs;
            for (uint32_t k = 0; k < M; k++) outs.emplace_back(flat.begin() + (size_t)k * frames, flat.begin() + (size_t)(k + 1) * frames);
            return outs;
        });
}

// ---- the way back from Firpfbch2Channelizer's rows to one stream (the synthesizer side of firpfbch2_crcf): M rows of `frames`
// values give frames M / 2 samples; behind the channelizer the stream comes back 2 M m - M / 2 + 1 samples late.  Kaiser prototype
// of cutoff fc (0: 0.5 / M, half the analyzer's); [empty], which the channelizer yields for an empty chunk, gives empty ----
inline Pipe<std::vector<Array<cf32>>, Array<cf32>> Firpfbch2Synthesizer(uint32_t M, uint32_t m, float as_db, float fc, uint32_t max_frames)
{
    return handlePipe<csdr_pfbsyn2, std::vector<Array<cf32>>, Array<cf32>>(
        [=](csdr_pfbsyn2 **h) { check(csdr_pfbsyn2_open_kaiser(M, m, as_db, fc, max_frames, h)); }, csdr_pfbsyn2_destroy,
        [M](csdr_pfbsyn2 *h, const std::vector<Array<cf32>> &rows) {
            const size_t frames = rows.empty() ? 0 : rows[0].size();
            if (!frames) return Array<cf32>{};
            if (rows.size() != M) throw std::runtime_error("Firpfbch2Synthesizer: not M rows");
            Array<cf32> flat;                                                // [M][frames]
            flat.reserve((size_t)M * frames);
            for (const auto &r : rows) {
                if (r.size() != frames) throw std::runtime_error("Firpfbch2Synthesizer: rows of unequal length");
                flat.insert(flat.end(), r.begin(), r.end());
            }
            Array<cf32> x(frames * (M / 2));
            uint32_t n = 0;
            check(csdr_pfbsyn2_process(h, reinterpret_cast<const float *>(flat.data()), (uint32_t)frames, reinterpret_cast<float *>(x.data()), &n));
            return x;
        });
}

// ---- rowResampler rate m as fc: the arbitrary-rate resampler (liquid's resamp_crcf for T = cf32, resamp_rrrf for T = float; the
// reference imports neither) on nchan rows that share one rate and one clock: every row of a chunk of n samples gives the same
// number of outputs, which the handle knows before the call; what turns the channelizers' fs / M into the whole number of
// samples per symbol the digital blocks take ----
template <class T> Pipe<Rows<T>, Rows<T>> RowResampler(double rate, uint32_t m, float as_db, float fc, uint32_t nchan, uint32_t max_in)
{
    return rowPipe<csdr_rowresamp, T, T>(
        "RowResampler", nchan,
        [=](csdr_rowresamp **h) { check(csdr_rowresamp_open(rate, m, as_db, fc, std::is_same<T, cf32>::value, nchan, max_in, h)); },
        csdr_rowresamp_destroy, [nchan](csdr_rowresamp *h, const Array<T> &x, uint32_t n) {
            uint32_t n_out = 0;
            check(csdr_rowresamp_count(h, n, &n_out));
            Array<T> y((size_t)nchan * n_out + 1);                       // + 1: a call that yields nothing still has a buffer
            check(csdr_rowresamp_process(h, reinterpret_cast<const float *>(x.data()), n, reinterpret_cast<float *>(y.data()), &n_out));
            return splitRows(y, nchan, n_out, n_out);
        });
}

template <class Out> Pipe<Array<cf32>, std::vector<Array<Out>>> fusedChain(const ChainOpts &o)
{
    return handlePipe<csdr_chain, Array<cf32>, std::vector<Array<Out>>>([o](csdr_chain **h) {
        csdr_chain_cfg cfg;
        csdr_chain_cfg_default(&cfg, o.channels);
        cfg.channels = o.channels; cfg.dc_block = o.dc_block; cfg.agc_threshold_db = o.agc;
        cfg.demod = o.fm ? CSDR_DEMOD_FM : (o.am ? CSDR_DEMOD_AM : (o.wbfm ? CSDR_DEMOD_WBFM : CSDR_DEMOD_NONE)); cfg.wbfm_decim = o.decim; cfg.deemph_fc = o.deemph_fc; cfg.kf = o.kf; cfg.mix = o.mix; cfg.max_frames = o.max_frames; cfg.flags = o.flags;
        cfg.device = o.device;
        if (o.world > 1) {
            if (o.channels % o.world || o.rank >= o.world) throw std::runtime_error("channel shards: world must divide the channel count");
            cfg.chan_first = o.rank; cfg.chan_stride = o.world;
        }
        check(csdr_chain_create(&cfg, h));
    }, csdr_chain_destroy, [o](csdr_chain *h, const Array<cf32> &a) {
        const uint32_t M = o.channels;
        if (a.empty()) return std::vector<Array<Out>>{Array<Out>{}};          // nx = 0 -> [empty] (Liquid.chs:856-862)
        uint32_t usable = (uint32_t)(a.size() / M * M), nf = usable / M;
        const bool mixed = o.mix && M > 1;
        const uint32_t no = o.wbfm ? nf / o.decim : nf;                        // DeWBFM: nf div decim samples per channel
        if (o.wbfm) { nf = no * o.decim; usable = nf * M; }                    // firDecimator drops the leftover (Liquid.chs:495-497)
        const uint32_t C = o.owned();                                          // rows this process produces
        Array<Out> flat((size_t)(mixed ? no : (size_t)C * no));
        uint32_t n_out = 0;
        if (usable) {
            // --mix across ranks: local left fold over the owned channels + one all-reduce (Trans.hs:119-122 over the node)
            if (mixed && o.comm) check(csdr_chain_process_mix(h, o.comm, reinterpret_cast<const float *>(a.data()), usable, flat.data(), &n_out));
            else check(csdr_chain_process(h, reinterpret_cast<const float *>(a.data()), usable, flat.data(), &n_out));
        }
        std::vector<Array<Out>> outs;
        if (mixed || M == 1) { outs.push_back(std::move(flat)); return outs; }
        for (uint32_t k = 0; k < C; k++) outs.emplace_back(flat.begin() + (size_t)k * no, flat.begin() + (size_t)(k + 1) * no);
        return outs;
    });
}

}  // namespace csdrhost

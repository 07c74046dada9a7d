"""Replay of `sdrProcess` / `assembleFold` (apps/SoapySDR.hs:181-283) for the file-input path:

    readFromFile chunksize fp        Source.chs:259-271   headerless LE float32 I/Q, <= chunksize samples per array
    | readFromAudioFile chunksize    Source.chs:273-307   a mono WAV / AU file: chunksize floats -> mixUp pi . realToComplex
      -> takeNArr n                  Trans.hs:33-56
      -> dcBlocker -> compact (4*nch*1024) -> PFB -> per-channel demod -> sinks   SoapySDR.hs:208-226

with the DSP behind `compact` done by the fused C-ABI chain.  Sinks are the reference's raw
`fileSink`s (Sink.hs:29-34): `<out>.cf32` / `<out>_ch<k>.cf32` for DeNo (SoapySDR.hs:240); demodulated audio goes to
raw `.f32` by default or, with `audio="AU" | "WAV"`, through `audioFileSink` (Sink.hs:41-74: libsndfile float,
big-endian; written here by hand, see the class).  `--offset` and `-b` are the reference's mixDown/mixUp and
resampler in front of `takeNArr`.  DeFMS (`demod="fms"`, SoapySDR.hs:261-264) skips the DC blocker, `compact` and the
channelizer: agc -> fmDemodulator 0.8 -> stereoFMDecoder per source chunk into one 2-channel sink.  DeNBFMSync k
(`demod="nbfmsync"`, SoapySDR.hs:273-280) runs the FM chain behind `compact (4*k*nch*1024)` and then symSyncR k 4 0 64 per
channel into raw `.f32` sinks."""
import struct
import numpy as np

from .pipes import (Chain, ChainConfig, SymSync, automaticGainControl, compose, fmDemodulator, idPipe, mixDown, mixUp, realToComplex,
                    resampler, stereoFMDecoder, unPipe)
from .trans import Fold, compact, mix as mix_pipe, takeNArr


def readFromFile(n, fp):
    """Source.chs:259-271: stream of arrays of at most n CF32 samples."""
    with open(fp, "rb") as f:
        while True:
            b = f.read(8 * n)
            if not b:
                return
            yield np.frombuffer(b[: len(b) // 8 * 8], dtype=np.complex64)


class SourceError(RuntimeError):
    """the reference's "Unable to open source" (SoapySDR.hs:172-179)"""


class AudioFile:
    """openAudioFile's SF.Handle (Source.chs:273-285) without libsndfile: a hand-written reader, as audioFileSink's writers are.

    RIFF / RIFX WAV with `fmt ` tag 1 (PCM 8 / 16 / 24 / 32), 3 (IEEE float 32 / 64) or 0xFFFE (extensible: the tag is the
    sub-format's first two bytes); chunks other than `fmt ` and `data` (fact, PEAK, LIST ...) are skipped.  `.snd` AU with
    encoding 2, 3, 4, 5 (PCM 8 / 16 / 24 / 32), 6, 7 (float 32 / 64), big-endian.  read(n) is libsndfile's float read
    (hGetBuffer): PCM16 / 32768, PCM24 / 8388608, PCM32 / 2147483648, WAV's unsigned 8 bit (v - 128) / 128, AU's signed
    8 bit / 128, floats as they are (64 -> 32 rounded).  A data size of 0 or 0xffffffff (a writer that never closed) means
    "to the end of the file"."""

    def __init__(self, path, f, channels, rate, kind, width, big, offset, nbytes):
        self.path, self.f, self.channels, self.rate = path, f, channels, rate
        self.kind, self.width, self.big = kind, width, big            # kind: "u8" | "int" | "float"
        self.left = nbytes // width * width
        f.seek(offset)

    @staticmethod
    def open(path):
        """the AudioFile of `path`, or None when the header is neither WAV nor AU (the caller then reads raw CF32, as
        initFileSource does when libsndfile refuses the file); SourceError for an audio file this reader cannot decode"""
        f = open(path, "rb")
        try:
            a = AudioFile._parse(path, f)
        except Exception:
            f.close()
            raise
        if a is None:
            f.close()
        return a

    @staticmethod
    def _parse(path, f):
        size = f.seek(0, 2)
        f.seek(0)
        head = f.read(12)
        if len(head) >= 12 and head[:4] in (b"RIFF", b"RIFX") and head[8:12] == b"WAVE":
            e = "<" if head[:4] == b"RIFF" else ">"
            fmt, pos = None, 12
            while pos + 8 <= size:
                f.seek(pos)
                cid, csz = struct.unpack(e + "4sI", f.read(8))
                if cid == b"fmt ":
                    b = f.read(min(csz, 40))
                    if len(b) < 16:
                        raise SourceError(f"Unable to open source: {path}: short fmt chunk")
                    tag, nch, rate, _, _, bits = struct.unpack(e + "HHIIHH", b[:16])
                    if tag == 0xFFFE and len(b) >= 26:
                        tag = struct.unpack(e + "H", b[24:26])[0]
                    fmt = (tag, nch, rate, bits)
                elif cid == b"data":
                    if fmt is None:
                        raise SourceError(f"Unable to open source: {path}: data chunk before fmt")
                    tag, nch, rate, bits = fmt
                    if (tag, bits) not in ((1, 8), (1, 16), (1, 24), (1, 32), (3, 32), (3, 64)):
                        raise SourceError(f"Unable to open source: {path}: WAV format tag {tag} with {bits} bits is not supported")
                    avail = size - (pos + 8)
                    nbytes = avail if csz in (0, 0xffffffff) else min(csz, avail)
                    kind = "float" if tag == 3 else ("u8" if bits == 8 else "int")
                    return AudioFile(path, f, nch, rate, kind, bits // 8, e == ">", pos + 8, nbytes)
                pos += 8 + csz + (csz & 1)
            raise SourceError(f"Unable to open source: {path}: WAV without a data chunk")
        if len(head) >= 4 and head[:4] == b".snd":
            f.seek(0)
            b = f.read(24)
            if len(b) < 24:
                raise SourceError(f"Unable to open source: {path}: short AU header")
            _, off, dsz, enc, rate, nch = struct.unpack(">4sIIIII", b)
            table = {2: ("int", 1), 3: ("int", 2), 4: ("int", 3), 5: ("int", 4), 6: ("float", 4), 7: ("float", 8)}
            if enc not in table or off < 24 or off > size:
                raise SourceError(f"Unable to open source: {path}: AU encoding {enc} is not supported")
            avail = size - off
            nbytes = avail if dsz in (0, 0xffffffff) else min(dsz, avail)
            return AudioFile(path, f, nch, rate, table[enc][0], table[enc][1], True, off, nbytes)
        return None

    def read(self, n):
        """hGetBuffer h n: up to n float32 samples (fewer at the end of the data, none after it)"""
        b = self.f.read(min(n * self.width, self.left))
        b = b[: len(b) // self.width * self.width]
        self.left -= len(b)
        e, w = (">" if self.big else "<"), self.width
        if self.kind == "float":
            return np.frombuffer(b, dtype=e + ("f4" if w == 4 else "f8")).astype(np.float32)
        if self.kind == "u8":
            return ((np.frombuffer(b, dtype=np.uint8).astype(np.int32) - 128).astype(np.float32) / np.float32(128.0))
        if w == 3:
            u = np.frombuffer(b, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
            hi, mid, lo = (u[:, 0], u[:, 1], u[:, 2]) if self.big else (u[:, 2], u[:, 1], u[:, 0])
            v = ((hi << 24) | (mid << 16) | (lo << 8)) >> 8               # sign-extended
        else:
            v = np.frombuffer(b, dtype=e + {1: "i1", 2: "i2", 4: "i4"}[w])
        return v.astype(np.float32) * np.float32(1.0 / float(1 << (8 * w - 1)))

    def close(self):
        self.f.close()


def openAudioFile(fp):
    """openAudioFile (Source.chs:273-285): the handle, or None for a file that is no audio file; anything but mono is the
    reference's SoapyException -> "Unable to open source" (there is no fall-back to raw for such a file)"""
    h = AudioFile.open(fp)
    if h is not None and h.channels != 1:
        h.close()
        raise SourceError(f"Unable to open source: {fp} has {h.channels} channels, an audio source must be mono")
    return h


def readFromAudioFile(n, h):
    """readFromAudioFile n (Source.chs:291-307) in front of its Pipe: arrays of at most n floats until the data ends"""
    while True:
        a = h.read(n)
        if a.size == 0:
            return
        yield a


def fileSource(chunksize, fp):
    """initFileSource (SoapySDR.hs:172-179): every file is tried as an audio file first and read as raw CF32 otherwise.
    Returns (stream of CF32 arrays, cleanup).  An audio source yields, per chunksize floats read,
    mixUp (2 pi 0.5) . realToComplex of them: chunksize / 2 samples, the real band 0 .. fs/2 on -fs/4 .. fs/4 of the complex
    rate fs / 2.  DEVIATION: the reference drops the last float of every chunk when chunksize is odd while liquid's windows
    run on; that is not replayed, an odd chunksize is refused for an audio source.  The last, short chunk of a file may be odd:
    its last float is dropped (firhilbDecim's `length div 2`)."""
    h = openAudioFile(fp)
    if h is None:
        return readFromFile(chunksize, fp), (lambda: None)
    if chunksize % 2:
        h.close()
        raise SourceError(f"Unable to open source: {fp} is an audio file and needs an even --chunksize (got {chunksize})")
    f = float(np.float32(2 * np.pi * 0.5))                             # the Haskell Float 2 * pi * 0.5
    process, cleanup = unPipe(compose(mixUp(f, max_samples=chunksize // 2), realToComplex(max_samples=chunksize // 2)))

    def done():
        h.close()
        cleanup()
    return process(readFromAudioFile(chunksize, h)), done


class fileSink(Fold):
    """Sink.hs:29-34: FS.writeChunks"""

    def __init__(self, path):
        self.f = open(path, "wb")

    def step(self, a):
        self.f.write(np.ascontiguousarray(a).tobytes())
        return self

    def done(self):
        self.f.close()


class _FusedFold(Fold):
    """addPipe fused (distribute_ sinks | sink): one chain call per compacted chunk, then the
    channel-major buffer is sliced exactly like Liquid.chs:850-862 and handed to sink k+1."""

    def __init__(self, chain, sinks, mixed):
        self.chain, self.sinks, self.mixed = chain, sinks, mixed

    def step(self, a):
        M = self.chain.M
        if len(a) == 0:
            self.sinks[0].step(a[:0])                 # nx = 0 -> [empty]: only sink 1 sees it
            return self
        usable = len(a) // M * M                      # a ragged stream tail cannot be channelized
        d = self.chain.decim                          # DeWBFM: firDecimator's n = length `div` m drops the leftover (Liquid.chs:495-497)
        if d > 1:
            usable = usable // (M * d) * (M * d)
            if usable == 0:
                for s in (self.sinks[:1] if (self.mixed or M == 1) else self.sinks):
                    s.step(np.empty(0, dtype=np.float32))
                return self
        y = self.chain.process(a[:usable])
        if self.mixed or M == 1:
            self.sinks[0].step(y.reshape(-1))
        else:
            for k, s in enumerate(self.sinks):
                s.step(y[k])
        return self

    def done(self):
        self.chain.close()
        for s in self.sinks:
            s.done()


class _SyncFold(Fold):
    """DeNBFMSync's fold behind `compact`: one chain call per compacted chunk (FM rows, no mix), then one symsync call over
    all rows (one stream per channel for the whole run); row k goes to sink k, or with -m the truncating left fold of the rows
    (Trans.hs:119-122) to the one sink."""

    def __init__(self, chain, sync, sinks, mixed):
        self.chain, self.sync, self.sinks, self.mixed = chain, sync, sinks, mixed

    def step(self, a):
        M = self.chain.M
        usable = len(a) // M * M
        if usable == 0:
            self.sinks[0].step(np.empty(0, dtype=np.float32))          # nx = 0 -> [empty]: only sink 1 sees it
            return self
        y = self.chain.process(a[:usable]).reshape(M, -1)
        rows = self.sync.process(y)
        if self.mixed:
            self.sinks[0].step(mix_pipe._process(None, rows))
        else:
            for s, r in zip(self.sinks, rows):
                s.step(r)
        return self

    def done(self):
        self.chain.close()
        self.sync.close()
        for s in self.sinks:
            s.done()


class audioFileSink(Fold):
    """audioFileSink fmt sr sn nch fp (Sink.hs:41-74): libsndfile, SampleFormatFloat, EndianBig, file fp + ".au" / ".wav".

    AU  : 24-byte header (".snd", data offset 24, data bytes, encoding 6 = 32-bit IEEE float, rate, channels), all
          big-endian, then big-endian floats -- what libsndfile's au_write_header leaves after close.
    WAV : libsndfile writes RIFX (big-endian WAV) for EndianBig with fmt (tag 3), fact and a PEAK chunk that holds a
          time stamp, so its bytes are not reproducible anyway; this writer emits RIFX + fmt + fact + data (no PEAK).
    libsndfile is not in the image: the layout is from the format definitions, unverified against the library."""

    def __init__(self, fmt, sr, sn, nch, fp):
        self.fmt, self.sr, self.nch = fmt.upper(), int(sr), int(nch)
        assert self.fmt in ("AU", "WAV")
        self.path = fp + (".au" if self.fmt == "AU" else ".wav")
        self.f = open(self.path, "wb")
        self.nbytes = 0
        self._header(0xffffffff if self.fmt == "AU" else 0)

    def _header(self, nbytes):
        self.f.seek(0)
        if self.fmt == "AU":
            self.f.write(struct.pack(">4sIIIII", b".snd", 24, nbytes, 6, self.sr, self.nch))
        else:
            frames = nbytes // (4 * self.nch)
            self.f.write(struct.pack(">4sI4s", b"RIFX", 4 + 24 + 12 + 8 + nbytes, b"WAVE"))
            self.f.write(struct.pack(">4sIHHIIHH", b"fmt ", 16, 3, self.nch, self.sr, self.sr * 4 * self.nch, 4 * self.nch, 32))
            self.f.write(struct.pack(">4sII", b"fact", 4, frames))
            self.f.write(struct.pack(">4sI", b"data", nbytes))

    def step(self, a):
        if len(a) == 0:
            return self
        b = np.ascontiguousarray(a, dtype=np.float32).astype(">f4").tobytes()
        self.f.write(b)
        self.nbytes += len(b)
        return self

    def done(self):
        self._header(self.nbytes)
        self.f.close()


def sdr_process(filename, channels=1, demod="none", kf=0.3, agc=0.0, mix=False, numsamples=1024,
                outname="output", chunksize=1024, m=4, offset=0.0, samplerate=2.56e6, bandwidth=0.0, decim=4, audio=None, k=4):
    """soapy-sdr --filename F -s samplerate -b bandwidth --offset f -c channels --demod ... -a agc [-m]
    -n numsamples -o outname.  demod="nbfmsync" is DeNBFMSync k.  Returns the list of files written."""
    if demod == "fms":
        return _sdr_process_fms(filename, channels, agc, numsamples, outname, chunksize, offset, samplerate, bandwidth, decim, audio)
    if demod == "nbfmsync":
        return _sdr_process_sync(filename, channels, agc, mix, numsamples, outname, chunksize, offset, samplerate, bandwidth, k)
    nch = channels
    mixed = bool(mix) and nch > 1
    source, close_source = fileSource(chunksize, filename)
    ext = ".cf32" if demod == "none" else ".f32"
    stems = [outname] if (mixed or nch == 1) else [f"{outname}_ch{k}" for k in range(1, nch + 1)]
    out_bw = bandwidth if bandwidth != 0 else samplerate
    if audio and demod != "none":
        # getAudioSink decim fmt chn (SoapySDR.hs:232-234): rate = round outBW `div` decim `div` nch, mono
        dec = decim if demod == "wbfm" else 1
        sinks = [audioFileSink(audio, int(round(out_bw)) // dec // nch, numsamples, 1, st) for st in stems]
        names = [sk.path for sk in sinks]
    else:
        names = [st + ext for st in stems]
        sinks = [fileSink(n) for n in names]
    # DeWBFM decim: de-emphasis corner 5000 / outBW, outBW = bandwidth or the sample rate (SoapySDR.hs:227-231, Liquid.chs:655)
    chain = Chain(ChainConfig(channels=nch, demod=demod, kf=kf, agc=agc, mix=mixed, max_frames=m * 1024, decim=decim,
                              deemph_fc=float(np.float32(5000.0 / out_bw))))
    fold = compact(m * nch * 1024, _FusedFold(chain, sinks, mixed))
    # prep = takeNArr ns . (resampler . offset)   (SoapySDR.hs:206-207)
    process, cleanup = unPipe(_prep(offset, samplerate, bandwidth, chunksize))       # (process, cleanup) <- unPipe (resampler . offset)
    try:
        for a in takeNArr(numsamples, process(source)):
            fold.step(a)
    finally:
        fold.done()
        cleanup()
        close_source()
    return names


def _prep(offset, samplerate, bandwidth, chunksize):
    """resampler . offset (SoapySDR.hs:190-205): per source chunk, the --offset mixer first (f = 2*pi*offset/fs; mixDown f if
    f > 0, mixUp (-f) if f < 0), then the resampler (rate = bandwidth / samplerate, 60 dB, identity when -b 0)"""
    f = np.float32(2 * np.pi * offset / samplerate)
    offset_p = idPipe
    if f != 0:
        offset_p = mixDown(float(f), max_samples=chunksize) if f > 0 else mixUp(float(-f), max_samples=chunksize)
    resamp_p = idPipe
    if bandwidth != 0:
        resamp_p = resampler(float(np.float32(bandwidth / samplerate)), 60.0, max_samples=chunksize)
    return compose(resamp_p, offset_p)


def _sdr_process_fms(filename, channels, agc, numsamples, outname, chunksize, offset, samplerate, bandwidth, decim, audio):
    """DeFMS decim fmt (SoapySDR.hs:261-264): prep src -> agc -> fmDemodulator 0.8 -> stereoFMDecoder outBW decim sink, one call
    per source chunk: no DC blocker, no compact, no channelizer; -c only divides the sink's rate.  The sink is one 2-channel
    audioFileSink at round(outBW) div decim div nch Hz (getAudioSink decim fmt 2), or raw interleaved L, R float32 <out>.f32."""
    out_bw = bandwidth if bandwidth != 0 else samplerate
    source, close_source = fileSource(chunksize, filename)
    if audio:
        sink = audioFileSink(audio, int(round(out_bw)) // decim // channels, numsamples, 2, outname)
        name = sink.path
    else:
        name = outname + ".f32"
        sink = fileSink(name)
    cap = 4 * chunksize + 16                                      # the resampler's largest output (rate <= 2: 2 ceil(r n))
    agc_p = automaticGainControl(agc, max_samples=cap) if agc != 0.0 else idPipe
    dem = compose(stereoFMDecoder(out_bw, decim, max_samples=cap), compose(fmDemodulator(0.8, max_samples=cap), agc_p))
    process, cleanup = unPipe(_prep(offset, samplerate, bandwidth, chunksize))
    r = dem._start()
    try:
        for a in takeNArr(numsamples, process(source)):
            sink.step(dem._process(r, a))
    finally:
        dem._done(r)
        sink.done()
        cleanup()
        close_source()
    return [name]


def _sdr_process_sync(filename, channels, agc, mix, numsamples, outname, chunksize, offset, samplerate, bandwidth, k):
    """DeNBFMSync k (SoapySDR.hs:273-280): assembleFold (fileSink (n ++ ".f32")) (fmDemWithSync k . agc) outname nch (4*k):
    prep -> dcBlocker -> compact (4*k*nch*1024) -> channelizer -> per channel agc -> fmDemodulator (0.02 k) -> symSyncR k 4 0 64
    -> raw .f32 sinks, or with -m the channels' truncating left fold into one sink"""
    nch = channels
    mixed = bool(mix) and nch > 1
    source, close_source = fileSource(chunksize, filename)
    stems = [outname] if (mixed or nch == 1) else [f"{outname}_ch{j}" for j in range(1, nch + 1)]
    names = [st + ".f32" for st in stems]
    sinks = [fileSink(nm) for nm in names]
    kf = float(np.float32(0.02) * np.float32(k))                   # 0.02 * fromIntegral k as a Haskell Float
    chain = Chain(ChainConfig(channels=nch, demod="fm", kf=kf, agc=agc, mix=False, max_frames=4 * k * 1024))
    sync = SymSync(k, 4, 0.0, 64, nchan=nch, max_samples=4 * k * 1024)
    fold = compact(4 * k * nch * 1024, _SyncFold(chain, sync, sinks, mixed))
    process, cleanup = unPipe(_prep(offset, samplerate, bandwidth, chunksize))
    try:
        for a in takeNArr(numsamples, process(source)):
            fold.step(a)
    finally:
        fold.done()
        cleanup()
        close_source()
    return names

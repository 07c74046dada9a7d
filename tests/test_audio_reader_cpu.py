"""The hand-written audio-file reader of the file source (composable_sdr_amd.app.AudioFile / openAudioFile, Source.chs:273-307):
WAV and AU headers, libsndfile's float normalisation, what audioFileSink writes, mono only, and raw CF32 left alone.  No GPU:
only the reader runs here."""
import struct

import numpy as np
import pytest

from composable_sdr_amd.app import AudioFile, SourceError, audioFileSink, openAudioFile, readFromAudioFile

f32 = np.float32


def _wav(path, tag, bits, nch, payload, rate=24000, endian="<", extra=b"", extensible=False):
    riff = b"RIFF" if endian == "<" else b"RIFX"
    if extensible:
        guid = struct.pack(endian + "H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
        fmt = struct.pack(endian + "HHIIHHHHI", 0xFFFE, nch, rate, rate * nch * bits // 8, nch * bits // 8, bits, 22, bits, 4) + guid
    else:
        fmt = struct.pack(endian + "HHIIHH", tag, nch, rate, rate * nch * bits // 8, nch * bits // 8, bits)
    body = b"WAVE" + b"fmt " + struct.pack(endian + "I", len(fmt)) + fmt + extra + b"data" + struct.pack(endian + "I", len(payload)) + payload
    open(path, "wb").write(riff + struct.pack(endian + "I", len(body)) + body)
    return str(path)


def _read_all(path, n=1000):
    h = openAudioFile(path)
    assert h is not None and h.channels == 1
    a = np.concatenate(list(readFromAudioFile(n, h)))
    assert h.read(n).size == 0
    h.close()
    return a


def test_pcm16_riff_with_unknown_chunks(tmp_path):
    rng = np.random.default_rng(1)
    v = rng.integers(-32768, 32768, 5001).astype("<i2")
    v[:2] = [-32768, 32767]
    junk = b"LIST" + struct.pack("<I", 5) + b"abcde\x00" + b"fact" + struct.pack("<II", 4, v.size)
    a = _read_all(_wav(tmp_path / "a.wav", 1, 16, 1, v.tobytes(), extra=junk))
    assert a.dtype == f32 and np.array_equal(a, v.astype(f32) / f32(32768.0))
    assert a[0] == -1.0


def test_pcm24_pcm32_and_u8(tmp_path):
    rng = np.random.default_rng(2)
    v = rng.integers(-(1 << 23), 1 << 23, 3000)
    v[:2] = [-(1 << 23), (1 << 23) - 1]
    b = (v & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    assert np.array_equal(_read_all(_wav(tmp_path / "b.wav", 1, 24, 1, b)), v.astype(f32) / f32(8388608.0))
    assert np.array_equal(_read_all(_wav(tmp_path / "bx.wav", 1, 24, 1, b, extensible=True)), v.astype(f32) / f32(8388608.0))
    w = rng.integers(-(1 << 31), 1 << 31, 3000).astype("<i4")
    assert np.array_equal(_read_all(_wav(tmp_path / "c.wav", 1, 32, 1, w.tobytes())), w.astype(f32) / f32(2147483648.0))
    u = rng.integers(0, 256, 999).astype(np.uint8)
    assert np.array_equal(_read_all(_wav(tmp_path / "d.wav", 1, 8, 1, u.tobytes())), (u.astype(f32) - 128) / 128)


def test_float32_and_float64_riff_bitwise(tmp_path):
    rng = np.random.default_rng(3)
    x = rng.standard_normal(4097).astype("<f4")
    a = _read_all(_wav(tmp_path / "e.wav", 3, 32, 1, x.tobytes()))
    assert np.array_equal(a.view(np.uint32), x.view(np.uint32))
    d = rng.standard_normal(100)
    assert np.array_equal(_read_all(_wav(tmp_path / "f.wav", 3, 64, 1, d.astype("<f8").tobytes())), d.astype(f32))


@pytest.mark.parametrize("fmt", ["WAV", "AU"])
def test_reads_back_what_audio_file_sink_writes(tmp_path, fmt):
    rng = np.random.default_rng(4)
    x = rng.standard_normal(2500).astype(f32)
    s = audioFileSink(fmt, 48000, 0, 1, str(tmp_path / "o"))
    s.step(x[:1000]).step(x[1000:])
    s.done()
    h = openAudioFile(s.path)
    assert (h.channels, h.rate, h.big) == (1, 48000, True)
    h.close()
    assert np.array_equal(_read_all(s.path).view(np.uint32), x.view(np.uint32))


def test_au_pcm16_and_an_unclosed_au(tmp_path):
    rng = np.random.default_rng(5)
    v = rng.integers(-32768, 32768, 777).astype(">i2")
    p = tmp_path / "g.au"
    open(p, "wb").write(struct.pack(">4sIIIII", b".snd", 32, v.size * 2, 3, 8000, 1) + b"annotate" + v.tobytes())
    assert np.array_equal(_read_all(str(p)), v.astype(f32) / f32(32768.0))
    x = rng.standard_normal(50).astype(">f4")
    q = tmp_path / "h.au"
    open(q, "wb").write(struct.pack(">4sIIIII", b".snd", 24, 0xffffffff, 6, 8000, 1) + x.tobytes())
    assert np.array_equal(_read_all(str(q)), x.astype(f32))


def test_short_reads_follow_the_chunk_size(tmp_path):
    v = np.arange(10, dtype="<i2")
    h = openAudioFile(_wav(tmp_path / "i.wav", 1, 16, 1, v.tobytes()))
    assert [a.size for a in readFromAudioFile(4, h)] == [4, 4, 2]
    h.close()


def test_stereo_is_refused_not_read_as_raw(tmp_path):
    v = np.zeros(64, "<i2")
    p = _wav(tmp_path / "j.wav", 1, 16, 2, v.tobytes())
    assert AudioFile.open(p).channels == 2
    with pytest.raises(SourceError, match="2 channels"):
        openAudioFile(p)
    q = tmp_path / "k.au"
    open(q, "wb").write(struct.pack(">4sIIIII", b".snd", 24, 64, 6, 8000, 2) + bytes(64))
    with pytest.raises(SourceError, match="2 channels"):
        openAudioFile(str(q))


def test_raw_cf32_is_not_taken_for_audio(tmp_path):
    rng = np.random.default_rng(6)
    x = (rng.standard_normal(512) + 1j * rng.standard_normal(512)).astype(np.complex64)
    p = tmp_path / "l.cf32"
    x.tofile(p)
    assert openAudioFile(str(p)) is None
    short = tmp_path / "m.cf32"
    open(short, "wb").write(b"RIF")
    assert openAudioFile(str(short)) is None

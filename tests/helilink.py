"""The synthetic helicopter downlink of README Example 6 that tests/test_helidecode_cpu.py and tests/test_audio_source_gpu.py
share: 40 position lines of 71 bytes, every byte sent as 8 data bits LSB first + "10", frames separated and bracketed by the
encoded ETX STX (which is the separator apps/HeliDecode.hs searches for).  Test infrastructure."""
import numpy as np

LINES = [(b"XY" + b"AN 52 12%02d\r\nBW 13 04%02d\r\n" % (30 + i, 10 + i)).ljust(71, b".") for i in range(40)]


def enc(data):
    """bytes -> bit string: 8 bits LSB first + '10' per byte"""
    return "".join("".join(str((b >> s) & 1) for s in range(8)) + "10" for b in data)


SEP = enc(b"\x03\x02")


def message_bits(seed=7, lead=333):
    """`lead` seeded random bits, then SEP line SEP line ... SEP"""
    rng = np.random.default_rng(seed)
    head = "".join(str(b) for b in rng.integers(0, 2, lead))
    return head + SEP + SEP.join(enc(ln) for ln in LINES) + SEP


def stream(bitstring, seed=8):
    """the synchroniser's output for these bits, idealised: +1.0 ('0') / -1.0 ('1') at the even samples, noise at the odd ones"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(2 * len(bitstring)).astype(np.float32)
    v[0::2] = [1.0 if c == "0" else -1.0 for c in bitstring]
    return v

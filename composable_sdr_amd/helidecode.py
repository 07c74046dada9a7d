"""Replay of `helidecode` (apps/HeliDecode.hs), the second program of README Example 6: it turns the `output.f32` that
`soapy-sdr --demod "DeNBFMSync 4"` writes (two synchronised samples per 1200-baud symbol) into the position fixes the
helicopter's downlink carries.  Host code only: one pass over a few thousand symbols, there is no hot path here.

    python -m composable_sdr_amd.helidecode output.f32 [outdir]      -> outdir/output.kml, outdir/output.m  (outdir: ".")

Line by line (HeliDecode.hs):
  main        :165-183   LE float32 in; bit '0' if v > 0 else '1'; every second sample (everyNth 2, :102-103)
  parseFrames :72-85     sepCap of  11000000 b b 01000000 b b  (ETX, STX as 8 data bits LSB first + 2 free bits): leftmost,
                         non-overlapping matches separate; the stretches between, before and behind them are candidates; those of
                         exactly 710 bits are frames
  decode      :87-100    groups of 10 bits, the first 8 LSB first; main drops the first 2 bytes of every frame: the line
  parseCoords :41-67     from the start of a line, zero or more of "AN " loc CRLF "BW " loc CRLF; loc = signed integer degrees,
                         optional white space, exactly two digits of minutes, signed integer hundredths of a minute
                         (sec = n / 100 * 60).  megaparsec semantics: a coordinate that fails before consuming anything ends
                         the list (text behind the last coordinate is ignored); one that fails inside makes the whole line
                         contribute nothing
  clean       :126-129   fix i is kept iff fix i + 1 exists and distKm(fix i + 1, fix i) < 0.1
  distKm      :108-124   as written there: (sin (d) / 2) ** 2, not sin (d / 2) ** 2; r = 6371; Float (float32) throughout
  toKML       :131-147   one Placemark per fix, <when> = running index, coordinates -lon, lat, 0 in degrees
  toOctave    :149-163   the first 20000 samples as `v(end+1) = ...;` between the reference's header and footer lines

The element structure and order of both files are the reference's.  The digits are not: Haskell's `printf "%f"` and
`"%12.4e"` of a Float cannot be checked without GHC, so the numbers are written as the shortest decimals that read back to
the same float32 (positional in the KML, scientific in the plot script).  The optional `outdir` argument is an addition; the
reference writes into the working directory."""
import os
import re
import sys

import numpy as np

f32 = np.float32

_SEP = re.compile("11000000[01][01]01000000[01][01]")
# megaparsec's `decimal` takes every digit there is and never gives one back: (?![0-9]) keeps the regex from backtracking into it
_LOC = r"([+-]?[0-9]+)(?![0-9])\s*([0-9][0-9])([+-]?[0-9]+)(?![0-9])"
_COORD = re.compile("AN " + _LOC + "\r\nBW " + _LOC + "\r\n")
FRAME_BITS = 710


def bits(samples):
    """main's bit string: '0' where v > 0 else '1', of samples 0, 2, 4, ..."""
    v = np.asarray(samples, f32).reshape(-1)[0::2]
    return "".join(np.where(v > 0, "0", "1"))


def frames(bitstring):
    """parseFrames: the stretches of exactly 710 bits between / around the separators"""
    out, pos = [], 0
    for m in _SEP.finditer(bitstring):
        out.append(bitstring[pos:m.start()])
        pos = m.end()
    out.append(bitstring[pos:])
    return [s for s in out if len(s) == FRAME_BITS]


def decode(frame):
    """decode + main's `drop 2 . fmap chr`: 10 bits per byte, the first 8 LSB first; the line behind the first 2 bytes (a str
    of code points 0 .. 255)"""
    by = []
    for i in range(0, len(frame), 10):
        by.append(sum(1 << s for s, c in enumerate(frame[i:i + 8]) if c != "0"))
    return "".join(chr(b) for b in by[2:])


def _loc(deg, mins, sec):
    """parseLoc: Loc deg mins ((sec / 100.0) * 60.0) in Float"""
    return (f32(int(deg)), f32(int(mins)), (f32(int(sec)) / f32(100.0)) * f32(60.0))


def parse_coords(lines):
    """parseCoords: [(lat, lon)], each a Loc (deg, min, sec) of float32"""
    out = []
    for s in lines:
        got, pos = [], 0
        while True:
            m = _COORD.match(s, pos)
            if m is None:
                # `many` stops quietly only where parseCoord fails without consuming: not at "AN ".  Behind "AN " it is an error,
                # and the line's list-monad result is empty.
                if s.startswith("AN ", pos):
                    got = []
                break
            got.append((_loc(*m.group(1, 2, 3)), _loc(*m.group(4, 5, 6))))
            pos = m.end()
        out.extend(got)
    return out


def to_deg(loc):
    """toDeg: deg + min / 60 + sec / 3600 in Float"""
    return f32(loc[0] + (loc[1] / f32(60.0)) + (loc[2] / f32(3600.0)))


def dist_km(ca, cb):
    """distKm ca cb, the reference's expression in float32"""
    rad = lambda d: (to_deg(d) * f32(np.pi)) / f32(180.0)  # noqa: E731
    lonra, lonrb, latra, latrb = rad(ca[1]), rad(cb[1]), rad(ca[0]), rad(cb[0])
    a = f32((np.sin(f32(latrb - latra)) / f32(2)) ** f32(2) +
            (np.cos(latra) * np.cos(latrb) * (np.sin(f32(lonrb - lonra)) / f32(2)) ** f32(2)))
    c = f32(2) * np.arctan2(np.sqrt(a), np.sqrt(f32(1) - a))
    return f32(f32(6371) * c)


def clean(coords):
    """clean: zip (tail cs) cs, keep the second of every pair closer than 0.1 km"""
    return [c for t, c in zip(coords[1:], coords) if dist_km(t, c) < f32(0.1)]


def _dec(v):
    return np.format_float_positional(f32(v), unique=True, trim="0")


def to_kml(path, coords):
    with open(path, "w") as f:
        f.write('<?xml version="1.0" encoding="UTF-8"?><kml xmlns="http://www.opengis.net/kml/2.2"><Document><name>Helo</name>\n')
        for n, c in enumerate(coords):
            f.write(f"<Placemark><TimeStamp><when>{n}</when></TimeStamp><Point><coordinates>{_dec(-to_deg(c[1]))},{_dec(to_deg(c[0]))},0"
                    "</coordinates></Point></Placemark>\n")
        f.write("</Document></kml>\n")


def to_octave(path, samples):
    base = os.path.splitext(os.path.basename(path))[0]
    lines = ["clear all; close all;", "k = 4; v = [];"]
    lines += ["v(end+1) = " + np.format_float_scientific(f32(v), unique=True, trim="0") + ";" for v in samples]
    lines += ["n = length(v); t = [0:(n-1)]/2; idx = 1:2:n;",
              "figure('color','white','position',[100 100 1200 400]);",
              "plot(t,v,'-','Color',[1 1 1]*0.6,...",
              "     t(idx),v(idx),'o','Color',[0 0.2 0.4]);",
              "axis([0 t(end) -2.5 2.5]); grid on;",
              "xlabel('Time [symbol index]'); ylabel('symsync output');",
              'print -dpng -color "-S1200,600" ' + base + ".png"]
    with open(path, "w") as f:
        f.write("".join(ln + "\n" for ln in lines))


def main(argv):
    """helidecode FILE [outdir]: writes outdir/output.m and outdir/output.kml; returns the cleaned fixes"""
    if not argv:
        raise SystemExit("usage: python -m composable_sdr_amd.helidecode output.f32 [outdir]")
    outdir = argv[1] if len(argv) > 1 else "."
    raw = open(argv[0], "rb").read()
    floats = np.frombuffer(raw[: len(raw) // 4 * 4], dtype="<f4")
    lines = [decode(fr) for fr in frames(bits(floats))]
    coords = clean(parse_coords(lines))
    to_octave(os.path.join(outdir, "output.m"), floats[:20000])
    to_kml(os.path.join(outdir, "output.kml"), coords)
    return coords


if __name__ == "__main__":
    main(sys.argv[1:])

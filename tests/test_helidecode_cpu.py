"""composable_sdr_amd.helidecode (apps/HeliDecode.hs) on a synthetic downlink built here: 333 seeded random bits, then 40
position lines, each byte as 8 data bits LSB first + "10", separated and bracketed by the encoded ETX STX, written as +-1.0 at
the even samples and noise at the odd ones.  helilink.py holds the generator (the GPU test of Example 6 sends the same message)."""
import re

import numpy as np

from composable_sdr_amd import helidecode as H
from helilink import LINES, SEP, enc, message_bits, stream

f32 = np.float32


def _lat(i):
    return 52 + 12 / 60 + (30 + i) * 0.6 / 3600


def _lon(i):
    return 13 + 4 / 60 + (10 + i) * 0.6 / 3600


def test_forty_frames_lines_fixes_and_kml(tmp_path):
    bs = message_bits()
    v = stream(bs)
    assert H.bits(v) == bs
    fr = H.frames(bs)
    assert len(fr) == 40 and all(len(f) == 710 for f in fr)
    lines = [H.decode(f) for f in fr]
    assert lines == [ln[2:].decode("latin-1") for ln in LINES]
    fixes = H.parse_coords(lines)
    assert len(fixes) == 40
    for i, (lat, lon) in enumerate(fixes):
        assert abs(float(H.to_deg(lat)) - _lat(i)) < 1e-5 and abs(float(H.to_deg(lon)) - _lon(i)) < 1e-5
    kept = H.clean(fixes)
    assert kept == fixes[:39]
    src = tmp_path / "output.f32"
    v.astype("<f4").tofile(src)
    assert H.main([str(src), str(tmp_path)]) == kept
    kml = open(tmp_path / "output.kml").read()
    assert kml.startswith('<?xml version="1.0" encoding="UTF-8"?><kml xmlns="http://www.opengis.net/kml/2.2"><Document><name>Helo</name>\n')
    assert kml.endswith("</Document></kml>\n")
    marks = re.findall(r"<Placemark><TimeStamp><when>(\d+)</when></TimeStamp><Point><coordinates>([^,]+),([^,]+),0</coordinates></Point></Placemark>\n", kml)
    assert len(marks) == 39 and kml.count("<Placemark>") == 39
    for i, (when, lon, lat) in enumerate(marks):
        assert int(when) == i
        assert abs(float(lon) + _lon(i)) < 1e-5 and abs(float(lat) - _lat(i)) < 1e-5
    m = open(tmp_path / "output.m").read().split("\n")
    assert m[:2] == ["clear all; close all;", "k = 4; v = [];"]
    body = [ln for ln in m if ln.startswith("v(end+1) = ")]
    assert len(body) == min(v.size, 20000)
    assert [f32(float(ln[11:-1])) for ln in body[:50]] == [f32(a) for a in v[:50]]
    assert m[-2] == 'print -dpng -color "-S1200,600" output.png' and m[-1] == ""


def test_a_frame_of_709_bits_is_dropped():
    good, short = enc(LINES[0]), enc(LINES[1])[:-1]
    assert len(good) == 710 and len(short) == 709
    bs = SEP + good + SEP + short + SEP + good + SEP
    assert H.frames(bs) == [good, good]
    assert H.frames(SEP + short + "0" + SEP) == [short + "0"]


def test_a_line_broken_inside_an_yields_no_fix():
    ok = "AN 52 1230\r\nBW 13 0410\r\n"
    assert len(H.parse_coords([ok + "....", ok + ok + "trailing text"])) == 3
    assert H.parse_coords(["....", ""]) == []                                # fails before consuming: an empty list, no error
    assert H.parse_coords([ok + "AN 52 1x30\r\nBW 13 0410\r\n"]) == []       # fails inside AN: the whole line contributes nothing
    assert H.parse_coords([ok + "AN 52 1230\r\nBX 13 0410\r\n"]) == []
    assert H.parse_coords(["AN 521230\r\nBW 13 0410\r\n"]) == []            # `decimal` swallows every digit, none left for the minutes
    (lat, lon), = H.parse_coords(["AN -7 0550\r\nBW +13\t 04-25\r\n"])
    assert lat == (f32(-7), f32(5), f32(30)) and lon == (f32(13), f32(4), f32(-15))


def test_two_fixes_one_km_apart_are_both_removed():
    a = ((f32(52), f32(12), f32(0)), (f32(13), f32(4), f32(0)))
    b = ((f32(52), f32(12), f32(32.4)), (f32(13), f32(4), f32(0)))         # 32.4" of latitude: 1.0 km
    assert 0.95 < float(H.dist_km(a, b)) < 1.05
    assert H.clean([a, b]) == []
    assert H.clean([a, a, b]) == [a]
    assert H.clean([]) == [] and H.clean([a]) == []

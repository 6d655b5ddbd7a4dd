"""The segment plan's numpy model (tests/tx_gso_util.py) against hand-derived vectors
(tests/golden/gso_vectors.json), and the library's host-only helpers against the model: the closed
form udpdk_gpu_tx_segment_span and the tile geometry. No GPU needed."""
import json
import os

import numpy as np
import pytest

import tx_gso_util as G
from udpdk_amd import abi

VEC = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gso_vectors.json")))


@pytest.mark.parametrize("v", VEC["span"], ids=lambda v: f"{v['len']}-{v['gso']}-{v['mtu']}")
def test_model_against_golden(v):
    segs = G.seg_lengths(v["len"], v["gso"])
    assert len(segs) == v["nseg"] and sum(segs) == v["len"]
    if v["segs"] is not None:
        assert segs == v["segs"]
    assert G.send_span(v["len"], v["gso"], v["mtu"]) == (v["span"], v["nseg"], v["nframes"])
    # the plan model places the same segments
    sends = G.make_sends([(16, v["len"], v["gso"], 0, 1, 2)])
    P = G.plan_model(sends, 16 + v["len"], v["nseg"] + 2, mtu=v["mtu"])
    assert P.stats["segments"] == v["nseg"] and P.stats["frames"] == v["nframes"]
    assert P.stats["bytes_needed"] == P.stats["end"] == v["span"] and P.stats["sends"] == 1
    assert list(P.payload_len[:v["nseg"]]) == segs and list(P.seg_off) == [0, v["nseg"]]
    assert list(P.sockfd[v["nseg"]:]) == [-1, -1] and list(P.frame_off[v["nseg"]:]) == [v["span"]] * 3
    assert list(P.payload_off[:v["nseg"]]) == [16 + t * v["gso"] for t in range(v["nseg"])]


@pytest.mark.parametrize("v", VEC["span"], ids=lambda v: f"{v['len']}-{v['gso']}-{v['mtu']}")
def test_library_span_against_golden(v):
    assert abi.tx_segment_span(v["len"], v["gso"], v["mtu"]) == (v["span"], v["nseg"], v["nframes"])


@pytest.mark.parametrize("mtu", [0, 576, 1500])
@pytest.mark.parametrize("gso", [0, 1, 7, 8, 1471, 1472, 1473, 65507])
def test_library_span_sweep(gso, mtu):
    """The closed form against the model, and against the sum of udpdk_gpu_tx_span over the model's
    segments, for every length 0..3000."""
    L = abi.lib()
    one = {}
    for ln in range(3001):
        segs = G.seg_lengths(ln, gso)
        want = G.send_span(ln, gso, mtu)
        assert abi.tx_segment_span(ln, gso, mtu) == want, (ln, gso, mtu)
        tot = nf_tot = 0
        for s in set(segs):
            if s not in one:
                nf = abi.C.c_uint32()
                one[s] = (int(L.udpdk_gpu_tx_span(s, mtu, abi.C.byref(nf))), nf.value)
            tot += one[s][0] * segs.count(s)
            nf_tot += one[s][1] * segs.count(s)
        assert (tot, len(segs), nf_tot) == want, (ln, gso, mtu)
    # NULL outputs are allowed
    assert L.udpdk_gpu_tx_segment_span(3000, gso, mtu, None, None) == G.send_span(3000, gso, mtu)[0]


def test_model_skip_precedence_and_tail():
    """Each rule alone, their precedence, and the out-of-room tail for both causes."""
    rows = [(0, 100, 10, -1, 1, 1),          # skipped
            (0, 65508, 0, 0, 1, 1),          # too_long
            (1000, 100, 10, 0, 1, 1),        # bad_range (the buffer is 1000 bytes)
            (0, 100, 1, 0, 1, 1),            # too_many with seg_limit 64
            (0, 65508, 0, -1, 1, 1),         # skipped before too_long
            (1000, 65508, 1, 0, 1, 1),       # too_long before bad_range and too_many
            (990, 100, 1, 0, 1, 1),          # bad_range before too_many
            (0, 100, 10, 0, 1, 1)]           # fine: 10 segments of 52 bytes
    P = G.plan_model(G.make_sends(rows), 1000, 64, seg_limit=64)
    assert P.reason == ["skipped", "too_long", "bad_range", "too_many", "skipped", "too_long", "bad_range", ""]
    assert P.stats["segments"] == 10 and P.stats["end"] == 520 and list(P.seg_off) == [0] * 8 + [10]
    three = G.make_sends([(0, 100, 10, 0, 1, 1)] * 3)
    P = G.plan_model(three, 1000, 25)                        # max_segs: the third send's last index is 29
    assert P.reason == ["", "", "no_room"] and list(P.seg_off) == [0, 10, 20, 20]
    assert P.stats["segs_needed"] == 30 and P.stats["bytes_needed"] == 1560 and P.stats["end"] == 1040
    P = G.plan_model(three, 1000, 64, out_cap=1039)          # out_cap: the second send ends at 1040
    assert P.reason == ["", "no_room", "no_room"] and P.stats["no_room"] == 2 and P.stats["end"] == 520
    assert list(P.sockfd[:11]) == [0] * 10 + [-1] and list(P.frame_off[9:12]) == [468, 520, 520]
    P = G.plan_model(three, 1000, 20, out_cap=1040)          # room ends exactly on a send boundary
    assert P.reason == ["", "", "no_room"] and P.stats["segments"] == 20


def test_geometry():
    B, S, nb, ns = abi.tx_segment_geometry(1, 1)
    assert B >= 64 and S >= 64 and B % 64 == 0 and S % 64 == 0 and (nb, ns) == (1, 1)
    assert abi.tx_segment_geometry(0, 0)[2:] == (1, 1)
    for k, m in ((B, S), (B + 1, S + 1), (5 * B - 1, 7 * S), (1 << 14, 1 << 20)):
        assert abi.tx_segment_geometry(k, m) == (B, S, -(-k // B), -(-m // S))
    u = abi.C.c_uint32()
    p = abi.C.byref(u)
    assert abi.lib().udpdk_gpu_tx_segment_geometry(1, 1, None, p, p, p) < 0
    assert abi.lib().udpdk_gpu_tx_segment_geometry(1, 1, p, p, p, None) < 0
    assert abi.GSO_MAX_SEGS == 64

"""The launch form of udpdk_gpu_rx, decided by rx_plan.h, checked without a GPU: build/rx_plan_check
(tools/rx_plan_check.cpp: the planner and the knob parser behind a main()) prints the form of a
row `n lanes fanout tail_recent KEY=VAL...`.

tests/golden/rx_plan_forms.json holds, per row, the classify<...> text and the form line that
UDPDK_RX_TRACE printed on an MI355X for that call, on zero-filled 64-byte frames, by the library
of the commit BEFORE the planner existed (udpdk_gpu_rx's decisions still inline in rx_on_pipe): the
planner must reproduce them byte for byte. tail_recent 1 was recorded after a batch of one
1500-byte frame on the same context, 0 on a fresh context. What no trace shows (lb, grids, LDS
bytes, rx_tile_base, the capacity refusals) is derived below by hand from that commit's source,
the derivation beside each row."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "build", "rx_plan_check")
GOLDEN = os.path.join(ROOT, "tests", "golden", "rx_plan_forms.json")


@pytest.fixture(scope="module")
def check():
    if not os.path.exists(CHECK):   # the driver's build() makes it (`make`: part of `all`)
        subprocess.run(["make", "build/rx_plan_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)

    def run(rows):
        out = subprocess.run([CHECK], input="\n".join(rows) + "\n", capture_output=True, text=True, check=True)
        lines = out.stdout.splitlines()
        assert len(lines) == len(rows), out.stdout + out.stderr
        return lines
    return run


def _recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_recorded_forms(check):
    """Every recorded row: the planner's two trace fragments equal the recorded ones."""
    rec = _recorded()
    assert len(rec) >= 100
    got = check([r["row"] for r in rec])
    bad = []
    for r, line in zip(rec, got):
        cls, form, rest = line.split(" | ")
        if (cls, form) != (r["classify"], r["form"]) or not rest.endswith(" rc 0"):
            bad.append((r["row"], r["classify"], r["form"], line))
    assert not bad, bad


def test_recording_covers_the_forms():
    """The recording holds every scan and scatter kind, both classify forms with and without the
    fused completion, and the fused-tile bound from both sides."""
    rec = {r["row"]: r for r in _recorded()}
    words = [dict(zip(r["form"].split()[0::2], r["form"].split()[1::2])) for r in rec.values()]
    assert {w["scan"] for w in words} == {"none", "cols512", "cols1024", "3pass"}
    assert {w["scatter"] for w in words} == {"fused", "compact1", "scatter1", "scatterw8", "scatterw16"}
    assert {r["classify"] for r in rec.values()} == {"classify<1>", "classify<2>", "classify<1> fused",
                                                      "classify<2> fused"}
    assert rec["4194304 1 1 0"]["form"].endswith("tiles 4096 mr 0 hist16 0 scan none scatter fused G 1")
    assert rec["4194305 1 1 0"]["form"].endswith("tiles 4097 mr 0 hist16 0 scan none scatter compact1 G 1")
    # the hint: a fresh context takes rx_classify<1> on one lane, a recent tail pass rx_classify<2>
    assert rec["1048576 1 1 0"]["classify"] == "classify<1> fused"
    assert rec["1048576 1 1 1"]["classify"] == "classify<2> fused"


# classify_lds_bytes(S, T, hist16) = DSC_OFF + 8 KiB x (T > 1024 ? 2 : 1) descriptor buffers
#   + 4 x hist words + 4 x min(T, 1024) verdict words + 4 KiB + 8 KiB,
# DSC_OFF = 4 waves x 3 x 64 x 4 + 4 x 16 x 4 = 3328; the span ring adds 4 x (2 x 256 + 16) x 4 = 8448.
DERIVED = [
    # the issue's three rows. 4096 lanes x 2^22: 2^22 / T x 4096 <= 2^21 first at T = 8192, 512 tiles
    # (mr: T > 1024); no fan-out: cols, hist16, rx_scatterw. G: 2 x 8192 = 16384 frames <= the group
    # bound, > 64 x 8 x 16 = 8192 so 16 waves, 8 x 16384 <= 2 x 16 x 4096, 256 workgroups >= 256:
    # G = 2; 4 x 8192 > 16384: stop. pick_lb(1024): 512 tiles / 16 per thread = 32 chunks, 1024 / 32
    # = 32 lanes, lb = 5, 4096 / 32 = 128 workgroups >= 128: cols1024, grid 128. LDS 3328 + 16384 +
    # 4 x 2048 (u16 pairs) + 4096 + 4096 + 8192 = 44288; no span (T > 1024).
    ("4194304 4096 1 0",
     "classify<2> | T 8192 tiles 512 mr 1 hist16 1 scan cols1024 scatter scatterw16 G 2 | "
     "lb 5 scan_grid 128 nc 0 lds 44288 compact_grid 0 tile_base 0 span 0 rc 0"),
    # 1024 lanes x 2^20: T = 1024 (2^20 <= 2^21), 1024 tiles. G: 2048 frames, 8 waves, 8 x 2048 =
    # 2 x 8 x 1024 (not above), 512 workgroups: G = 2; 4096 frames: 32768 > 16384: stop.
    # pick_lb(1024): 64 chunks, 16 lanes, lb 4, 64 workgroups < 128: lb 3 (128 workgroups; the floor):
    # < 4, so rx_scan_cols<512>: 32 chunks, 16 lanes, lb 4 -> 3, grid 128. LDS 3328 + 8192 + 4 x 512
    # + 4096 + 4096 + 8192 = 29952, + 8448 (span: G 2 form, one-round tiles) = 38400.
    ("1048576 1024 1 0",
     "classify<2> | T 1024 tiles 1024 mr 0 hist16 1 scan cols512 scatter scatterw8 G 2 | "
     "lb 3 scan_grid 128 nc 0 lds 38400 compact_grid 0 tile_base 0 span 1 rc 0"),
    ("1048576 1024 1 0 UDPDK_RX_SPAN=0",
     "classify<2> | T 1024 tiles 1024 mr 0 hist16 1 scan cols512 scatter scatterw8 G 2 | "
     "lb 3 scan_grid 128 nc 0 lds 29952 compact_grid 0 tile_base 0 span 0 rc 0"),
    # one lane x 2^20, fresh hints: speculative entries, 1024 tiles <= 4096: fused, rx_classify<1>, no
    # other launch. LDS 3328 + 8192 + 4 x 4 + 4096 + 4096 + 8192 = 27920 (no span: G 1 form).
    ("1048576 1 1 0",
     "classify<1> fused | T 1024 tiles 1024 mr 0 hist16 0 scan none scatter fused G 1 | "
     "lb 0 scan_grid 0 nc 0 lds 27920 compact_grid 0 tile_base 0 span 0 rc 0"),
    # ... UDPDK_RX_FUSE=0: rx_compact1 on min(1024 tiles, 256) workgroups, 1024 <= 4096 tiles: no rx_tile_base
    ("1048576 1 1 0 UDPDK_RX_FUSE=0",
     "classify<1> | T 1024 tiles 1024 mr 0 hist16 0 scan none scatter compact1 G 1 | "
     "lb 0 scan_grid 0 nc 0 lds 27920 compact_grid 256 tile_base 0 span 0 rc 0"),
    # one lane x 2^23: 8192 tiles > 4096: not fused; > COMPACT1_DIRECT_TILES and <= partial_cap
    # ((2^21 + 1) / 32 + 2): rx_tile_base runs
    ("8388608 1 1 0",
     "classify<1> | T 1024 tiles 8192 mr 0 hist16 0 scan none scatter compact1 G 1 | "
     "lb 0 scan_grid 0 nc 0 lds 27920 compact_grid 256 tile_base 1 span 0 rc 0"),
    # ... without speculative entries (2048-frame tiles): one rx_compact1 workgroup per tile;
    # rx_classify<2> after a tail pass, its span sweep only on one-round tiles
    ("8388608 1 1 1 UDPDK_ONE_LANE_TILE=2048",
     "classify<2> | T 2048 tiles 4096 mr 1 hist16 0 scan none scatter compact1 G 1 | "
     "lb 0 scan_grid 0 nc 0 lds 36112 compact_grid 4096 tile_base 0 span 0 rc 0"),
    # 600 lanes x 2^20: T = 1024, 1024 tiles. G: 8 x 2048 > 2 x 8 x 600: G = 1. pick_lb(1024): lb 4,
    # 38 workgroups < 128: lb 3, and the floor of 8 lanes holds it there (75 workgroups < 128);
    # rx_scan_cols<512> likewise: lb 3, grid 75. LDS 3328 + 8192 + 4 x 300 + 4096 + 4096 + 8192 + 8448.
    ("1048576 600 1 0",
     "classify<2> | T 1024 tiles 1024 mr 0 hist16 1 scan cols512 scatter scatterw8 G 1 | "
     "lb 3 scan_grid 75 nc 0 lds 37552 compact_grid 0 tile_base 0 span 1 rc 0"),
    # the 3-pass scan: 1024 tiles / 32 per chunk = 32 chunks per lane; u32 histogram (4 x 1024 bytes)
    ("1048576 1024 1 0 UDPDK_RX_SCAN_COLS_TILES=0",
     "classify<2> | T 1024 tiles 1024 mr 0 hist16 0 scan 3pass scatter scatterw8 G 2 | "
     "lb 0 scan_grid 0 nc 32 lds 40448 compact_grid 0 tile_base 0 span 1 rc 0"),
]

# The capacity refusals (-EINVAL = -22), each from both sides of its bound.
REFUSALS = [
    # lanes x tiles > hist_cap: 4096 lanes x 2^20 frames: T = 2048, 512 tiles, 2^21 entries
    ("1048576 4096 1 0 hist_cap=2097151", -22), ("1048576 4096 1 0 hist_cap=2097152", 0),
    # tiles > tiles_cap
    ("1048576 1 1 0 tiles_cap=1023", -22), ("1048576 1 1 0 tiles_cap=1024", 0),
    # a context of 1024 frames x 16 lanes: tiles_cap = 1024 / 1024 + 1 = 2 < 512 tiles
    ("4194304 4096 1 0 max_frames=1024 max_lanes=16", -22),
    # 3-pass scan, chunks x lanes > partial_cap: 32 x 1024
    ("1048576 1024 1 0 UDPDK_RX_SCAN_COLS_TILES=0 partial_cap=32767", -22),
    ("1048576 1024 1 0 UDPDK_RX_SCAN_COLS_TILES=0 partial_cap=32768", 0),
]


def test_derived_rows(check):
    got = check([r for r, _ in DERIVED])
    for (row, want), line in zip(DERIVED, got):
        assert line == want, row


def test_derived_rows_agree_with_the_recording():
    """Where a hand-derived row was also recorded, the recording has the last word."""
    rec = {r["row"]: r for r in _recorded()}
    both = [(row, want) for row, want in DERIVED if row in rec]
    assert len(both) >= 6
    for row, want in both:
        assert want.split(" | ")[:2] == [rec[row]["classify"], rec[row]["form"]], row


def test_capacity_refusals(check):
    got = check([r for r, _ in REFUSALS])
    for (row, rc), line in zip(REFUSALS, got):
        assert line.endswith(f" rc {rc}"), (row, line)


DEFAULT_KNOBS = {"one_lane_tile": 0, "geo_cap": 1 << 21, "force_fuse": -1, "force_tailg": 0, "force_mr": -1,
                 "no_span": 0, "policy": 1, "trace": 0, "scan_cols_tiles": 16384, "no_inline": 0,
                 "scatter_group_frames": 16384, "scatter_min_wg": 256, "tx_parts": 0, "tx_grid": 4096,
                 "gather_grid": 16384}
# environment -> the knobs that differ from the defaults
KNOB_ROWS = [
    ("", {}),
    ("UDPDK_ONE_LANE_TILE=3000", {}),                            # not a power of two: ignored
    ("UDPDK_ONE_LANE_TILE=512", {}),                             # below a round: ignored
    ("UDPDK_ONE_LANE_TILE=16384", {}),
    ("UDPDK_ONE_LANE_TILE=4096", {"one_lane_tile": 4096}),
    ("UDPDK_RX_SCAN_COLS_TILES=-5", {"scan_cols_tiles": 0}),     # clamped
    ("UDPDK_RX_SCAN_COLS_TILES=99999", {}),                      # clamped to 16384
    ("UDPDK_RX_SCAN_COLS_TILES=100", {"scan_cols_tiles": 100}),
    ("UDPDK_RX_HIST_CAP=1000", {}),                              # below 2^16: ignored
    ("UDPDK_RX_HIST_CAP=134217728", {}),                         # above 2^26: ignored
    ("UDPDK_RX_HIST_CAP=0x10000", {"geo_cap": 65536}),           # strtoull, base 0
    ("UDPDK_RX_TAILG=3", {}),                                    # ignored
    ("UDPDK_RX_TAILG=2", {"force_tailg": 2}),
    ("UDPDK_TX_PARTS=9", {"tx_parts": 4}),                       # clamped
    ("UDPDK_TX_PARTS=0", {"tx_parts": 1}),
    ("UDPDK_TX_GRID=0", {"tx_grid": 1}),
    ("UDPDK_GATHER_GRID=-3", {"gather_grid": 1}),
    ("UDPDK_RX_FUSE=0 UDPDK_RX_MR=7 UDPDK_RX_SPAN=0 UDPDK_RX_POLICY=0 UDPDK_RX_TRACE= UDPDK_RX_NO_INLINE=0",
     {"force_fuse": 0, "force_mr": 1, "no_span": 1, "policy": 0, "trace": 1, "no_inline": 1}),
    ("UDPDK_RX_SPAN=x UDPDK_RX_FUSE=x", {"no_span": 1, "force_fuse": 0}),   # atoi("x") = 0
    ("UDPDK_SCATTER_GROUP_FRAMES=8192 UDPDK_SCATTER_MIN_WG=1", {"scatter_group_frames": 8192, "scatter_min_wg": 1}),
]


def test_knob_parsing(check):
    got = check([f"knobs {env}" for env, _ in KNOB_ROWS])
    for (env, diff), line in zip(KNOB_ROWS, got):
        w = line.split()
        assert dict(zip(w[0::2], (int(x) for x in w[1::2]))) == dict(DEFAULT_KNOBS, **diff), env

"""bench.py on the GPU at a small batch: a plain run times exactly --steps steps and reports
only the headline figures; --dump-outputs writes the last timed step's verdict words and lanes,
equal to the oracle's for the same frames and the same from run to run; --full adds the GPU-event
and per-kernel figures. One bench process per case, 4096 frames, no rotation."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
N = 4096
SMALL = ["--gpus", "1", "--frames", str(N), "--rotate-mib", "0"]
FULL_ONLY = ("gpu_us_per_step", "single_call_us", "depth1", "kernel_us", "roofline", "scale", "strong",
             "other_configs", "end_to_end", "socket_path", "tx", "reassembly", "rss", "gather")


def _bench(args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH] + SMALL + args, capture_output=True, text=True,
                       timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("config", [2, 4])
def test_plain_run_and_dumped_outputs(config, tmp_path):
    import oracle as O
    from udpdk_amd import frames as F
    line = _bench(["--steps", "3", "--warmup", "2", "--config", str(config),
                   "--dump-outputs", str(tmp_path / "a")])
    assert line["steps"] == 3 and line["warmup"] == 2 and line["full"] is False
    assert line["unit"] == "Mpkt/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    # value is the frames of the timed steps over their time (ms_per_step is rounded to 1e-5 ms:
    # at most 0.5 % of a step that launches two kernels and so takes more than a microsecond)
    assert line["value"] == pytest.approx(N / line["ms_per_step"] / 1e3, rel=1e-2)
    assert line["cpu_baseline"] is None and not [k for k in FULL_ONLY if k in line]
    w = F.config_batch(config, n=N, shard=0)
    b = w.batch
    meta, loff, pkt, _ = O.rx(O.bindtable_from_lists(w.port_lists()), b.frames, b.frames_bytes,
                              b.offset, b.length, None, w.n_sockets)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("meta", "lane_off", "lane_pkt")}
    assert sorted(os.listdir(tmp_path / "a")) == ["lane_off.npy", "lane_pkt.npy", "meta.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["meta"], meta.astype(np.float64))
    assert np.array_equal(got["lane_off"], loff.astype(np.float64))
    assert np.array_equal(got["lane_pkt"], np.asarray(pkt)[:int(loff[-1])].astype(np.float64))
    if config == 2:
        # the same arguments again: the same inputs, so the same outputs
        _bench(["--steps", "3", "--warmup", "2", "--config", str(config),
                "--dump-outputs", str(tmp_path / "b")])
        for k, a in got.items():
            assert np.array_equal(a, np.load(tmp_path / "b" / f"{k}.npy")), k


@pytest.mark.gpu
def test_full_run_adds_kernel_figures():
    line = _bench(["--full", "--steps", "4", "--warmup", "2", "--timing-every", "1", "--no-scale",
                   "--no-strong", "--no-cpu-baseline", "--no-extra"])
    assert line["full"] is True and line["steps"] == 4
    assert line["gpu_us_per_step"] > 0 and line["single_call_us"] > 0
    assert line["kernel_us"]["rx_classify"] > 0
    assert line["roofline"]["kernel"] == "rx_classify" and line["roofline"]["achieved"] > 0
    assert "scale" not in line and "strong" not in line and "other_configs" not in line

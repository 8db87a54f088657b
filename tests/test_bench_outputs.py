"""bench.py's plain run, ``--full`` and ``--dump-outputs``.

CPU: the threaded weight generator equals whisper.synthetic's serial one, the dump writes
float64 arrays of the segment records, the options parse.  GPU: one plain and one
``--full`` run of the micro model (two 30 s windows): the plain line carries the headline
fields and none of the figures that take runs of their own, ``--steps`` sets the timed
steps, and two runs with the same arguments dump the same segment records."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("roofline", "roofline_cross_attn", "roofline_step", "latency_1window", "cpu_baseline")
DUMPED = bench.SEGMENT_SCALARS + ("n_tokens", "tokens")


def test_seeded_state_dict_equals_serial_generator():
    from whisper import synthetic as S
    dims = S.MODEL_DIMS["micro"]
    ref = S.synthetic_state_dict(dims, 0)
    got = bench.seeded_state_dict(dims, 0)
    assert list(got) == list(ref)
    for k in ref:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k


def test_dump_outputs_writes_float_arrays(tmp_path):
    segs = [dict(id=0, seek=0, start=0.0, end=2.5, text="a", tokens=[50364, 7, 8, 50489], temperature=0.0,
                 avg_logprob=-0.25, compression_ratio=1.5, no_speech_prob=0.125),
            dict(id=1, seek=3000, start=30.0, end=31.0, text="b", tokens=[50364, 9], temperature=0.0,
                 avg_logprob=-0.5, compression_ratio=0.75, no_speech_prob=0.5)]
    out = tmp_path / "nested" / "dir"
    bench.dump_outputs(str(out), segs)
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in DUMPED)
    arrays = {k: np.load(out / (k + ".npy")) for k in DUMPED}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert arrays["seek"].tolist() == [0.0, 3000.0]
    assert arrays["avg_logprob"].tolist() == [-0.25, -0.5]
    assert arrays["n_tokens"].tolist() == [4.0, 2.0]
    assert arrays["tokens"].tolist() == [[50364.0, 7.0, 8.0, 50489.0], [50364.0, 9.0, -1.0, -1.0]]


def test_dump_outputs_of_no_segments(tmp_path):
    bench.dump_outputs(str(tmp_path), [])
    assert np.load(tmp_path / "tokens.npy").shape == (0, 0)
    assert np.load(tmp_path / "seek.npy").shape == (0,)


def test_options(monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, "")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
    assert "--steps" in capsys.readouterr().err


def _bench(extra, out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--model", "micro", "--seconds", "60", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(out_dir)] + extra,
                       capture_output=True, text=True, timeout=280, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, p.stdout
    return lines[0], {k: np.load(os.path.join(out_dir, k + ".npy")) for k in DUMPED}


@pytest.mark.gpu
def test_plain_and_full_run(tmp_path):
    plain, a = _bench([], tmp_path / "plain")
    assert all(k in plain for k in HEADLINE), sorted(plain)
    assert not any(k in plain for k in FULL_ONLY), sorted(plain)
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["higher_is_better"] is True
    assert plain["ms_per_step"] > 0
    # value is the audio seconds of the timed steps over their wall time, ms_per_step that wall time per step
    assert plain["value"] == pytest.approx(60.0 / (plain["ms_per_step"] * 1e-3), rel=1e-2)
    # two 30 s windows, every segment of them
    assert set(a["seek"].tolist()) == {0.0, 3000.0}
    assert a["tokens"].shape[0] == a["seek"].shape[0] == a["n_tokens"].shape[0]
    assert sum(x.nbytes for x in a.values()) <= 64 << 20

    full, b = _bench(["--full", "--cpu-steps", "4"], tmp_path / "full")
    assert all(k in full for k in HEADLINE + FULL_ONLY), sorted(full)
    assert full["metric"] == plain["metric"] and full["unit"] == plain["unit"] and full["dtype"] == plain["dtype"]
    assert full["cpu_baseline"].get("value"), full["cpu_baseline"]
    # same arguments, same inputs: the same windows and the same tokens of each segment
    assert np.array_equal(a["seek"], b["seek"]) and np.array_equal(a["tokens"], b["tokens"])

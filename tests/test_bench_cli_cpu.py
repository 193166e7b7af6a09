"""bench.py's command-line contract on a machine without the GPUs it is asked for: `--gpus N`
(no launcher) must refuse with exit status 2 instead of reporting a smaller run as N GPUs."""
from __future__ import annotations

import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_more_gpus_than_visible_exits_2():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--steps", "1", "--warmup", "0",
                        "--no-config3", "--md-timeout", "120"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, cwd=ROOT)
    assert r.returncode == 2, r.stderr.decode(errors="replace")[-2000:]
    err = r.stderr.decode(errors="replace")
    assert "refusing to report" in err
    assert not r.stdout.strip(), "no bench line may be printed"


def test_plain_run_drops_every_side_measurement(monkeypatch):
    """Without --full every check and side measurement is off; --full leaves the --no-* switches alone."""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_parity and a.no_config3 and a.no_config5 and a.no_cpu_baseline and a.no_pmc
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-pmc", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.no_pmc and a.dump_outputs == "d"
    assert not (a.no_parity or a.no_config3 or a.no_config5 or a.no_cpu_baseline)


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: float64 arrays, the groups in the order received, integer results as their
    value and floating ones from their bits; the same result gives the same files."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    groups = [(5, np.array([1000, 2000], np.int64), np.array([1.5, float("nan")], np.float64).view(np.uint64),
               np.zeros(2, np.uint8)),
              (2, np.array([1000], np.int64), np.array([-7], np.int64).view(np.uint64), np.ones(1, np.uint8))]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), bench.result_copy(groups))
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["group_id", "group_index", "group_len", "is_int", "point_index", "timestamp_ms", "value"]
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["group_id"].tolist() == [5, 2] and got["group_len"].tolist() == [2, 1]
    assert got["group_index"].tolist() == [0, 1]
    assert got["timestamp_ms"].tolist() == [1000, 2000, 1000] and got["is_int"].tolist() == [0, 0, 1]
    assert got["point_index"].tolist() == [0, 1, 2]
    np.testing.assert_array_equal(got["value"], [1.5, float("nan"), -7.0])
    for k, v in got.items():
        assert v.tobytes() == np.load(tmp_path / "b" / (k + ".npy")).tobytes()


def test_dump_outputs_samples_a_large_result(tmp_path, monkeypatch):
    """Past the caps the dump is a fixed, sorted, repeatable sample: point_index / group_index name
    the positions kept, and the per-point and per-group arrays hold exactly those positions."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_POINTS", 4)
    monkeypatch.setattr(bench, "DUMP_MAX_GROUPS", 2)
    vals = np.arange(12, dtype=np.float64) * 0.5 + 1
    groups = [(10 + g, np.arange(3, dtype=np.int64) * 1000 + g, vals[3 * g:3 * g + 3].view(np.uint64), np.zeros(3, np.uint8))
              for g in range(4)]
    all_ts = np.concatenate([t for _, t, _, _ in groups]).astype(np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), bench.result_copy(groups))
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    pi = a["point_index"].astype(int)
    assert len(pi) == 4 and len(set(pi)) == 4 and list(pi) == sorted(pi) and 0 <= pi[0] and pi[-1] < 12
    assert pi.tolist() == np.sort(np.random.default_rng(0x5EED).choice(12, 4, replace=False)).tolist()
    np.testing.assert_array_equal(a["value"], vals[pi])
    np.testing.assert_array_equal(a["timestamp_ms"], all_ts[pi])
    assert a["is_int"].tolist() == [0, 0, 0, 0]
    gi = a["group_index"].astype(int)
    assert len(gi) == 2 and len(set(gi)) == 2 and list(gi) == sorted(gi) and gi[-1] < 4
    assert a["group_id"].tolist() == [10 + g for g in gi] and a["group_len"].tolist() == [3, 3]

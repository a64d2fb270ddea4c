"""`python bench.py --gpus N` without WORLD_SIZE launches its N ranks itself: the parent starts
torch.distributed.run as a child process, relays rank 0's JSON line and the exit code, and never touches the GPU."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "helpers", "fake_rank.py")


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def test_spawn_ranks_relays_arguments_and_the_json_line(capfd):
    rc, line = _bench().spawn_ranks(2, ["--gpus", "2", "--steps", "3"], script=FAKE)
    assert rc == 0
    got = json.loads(line)
    assert got["argv"] == ["--gpus", "2", "--steps", "3"]
    assert got["world"] == 2 and got["master_addr"] == "127.0.0.1" and got["local_rank"] == 0
    assert line in capfd.readouterr().out  # relayed to the parent's stdout as well


def test_spawn_ranks_relays_a_failing_rank():
    rc, _ = _bench().spawn_ranks(2, ["--exit-code", "7"], script=FAKE)
    assert rc != 0


def test_plain_invocation_does_not_import_torch_cuda_in_the_parent():
    """The parent branch sits in front of every torch import of main(): run bench.py --gpus 2 with the rank script swapped
    for the fake through the launcher's own function, in a subprocess whose torch import is poisoned."""
    code = (
        "import sys, types, json\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "import bench\n"
        "assert 'torch' not in sys.modules\n"
        f"rc, line = bench.spawn_ranks(2, ['--steps', '1'], script={FAKE!r})\n"
        "assert 'torch' not in sys.modules\n"
        "sys.exit(rc)\n"
    )
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_dump_outputs_writes_the_scores_and_a_seeded_sample_above_the_cap(tmp_path, monkeypatch):
    """--dump-outputs: float32 scores as DIR/<name>.npy; above DUMP_MAX_BYTES a fixed sample of whole users, their rows
    beside them, the same sample on every run."""
    import numpy as np

    bench = _bench()
    scores = np.random.default_rng(3).standard_normal((128, 101))
    bench.dump_outputs(str(tmp_path / "full"), "scores", scores)
    got = np.load(tmp_path / "full" / "scores.npy")
    assert got.dtype == np.float32 and np.array_equal(got, scores.astype(np.float32))
    assert not (tmp_path / "full" / "scores_rows.npy").exists()

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10_000)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), "scores", scores)
    sample, rows = np.load(tmp_path / "a" / "scores.npy"), np.load(tmp_path / "a" / "scores_rows.npy")
    assert sample.nbytes + rows.nbytes <= 10_000 and len(rows) > 0 and rows.dtype == np.float64
    assert np.array_equal(sample, scores.astype(np.float32)[rows.astype(np.int64)])
    assert np.array_equal(sample, np.load(tmp_path / "b" / "scores.npy"))
    assert np.array_equal(rows, np.load(tmp_path / "b" / "scores_rows.npy"))

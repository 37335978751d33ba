"""bench.py's command line: `--gpus N` must either start N ranks itself or fail loudly; `--dump-outputs`
writes the last timed step's results."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=240):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_world_size_that_disagrees_with_gpus_is_refused():
    r = _run(["--gpus", "2"], {"WORLD_SIZE": "1"})
    assert r.returncode != 0
    assert "--gpus 2 but WORLD_SIZE=1" in (r.stdout + r.stderr)


def test_gpus_n_without_a_launcher_starts_n_ranks():
    """No launcher in the environment: bench.py starts a child torch.distributed.run with N ranks
    before touching any GPU and exits with its code.  Here (no GPU) both ranks stop at the
    'no HIP device' check, which is the product's no-CPU-fallback rule."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the ranks would run the whole benchmark")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    out = r.stdout + r.stderr
    assert r.returncode != 0
    assert "needs an MI355X" in out
    assert "local_rank: 1" in out or "rank      : 1" in out or out.count("needs an MI355X") >= 2


def test_dump_outputs_writes_exact_arrays_and_a_seeded_sample_under_the_cap(tmp_path, monkeypatch):
    """--dump-outputs' writer: integers as float64 and floats as float32, exactly; above the cap the same
    seeded sample of rows every time, named by query_rows.npy, with the files (headers included) under it."""
    import numpy as np
    import bench
    rng = np.random.default_rng(1)
    nq, k = 1024, 11
    arrays = {"doc_ids": rng.integers(0, 2 ** 32 - 1, (nq, k), dtype=np.uint32),
              "scores": rng.random((nq, k), dtype=np.float32), "counts": rng.integers(0, k + 1, nq).astype(np.uint32)}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    assert np.array_equal(np.load(tmp_path / "all" / "query_rows.npy"), np.arange(nq, dtype=np.float64))
    for name, a in arrays.items():
        got = np.load(tmp_path / "all" / f"{name}.npy")
        assert got.dtype == (np.float32 if a.dtype.kind == "f" else np.float64)
        assert np.array_equal(got, a)
    cap = 64 * 1024
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", cap)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays)
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= cap
    rows = np.load(tmp_path / "s1" / "query_rows.npy")
    assert 0 < len(rows) < nq and np.array_equal(rows, np.load(tmp_path / "s2" / "query_rows.npy"))
    assert np.array_equal(np.load(tmp_path / "s1" / "doc_ids.npy"), arrays["doc_ids"][rows.astype(np.int64)])


@pytest.mark.gpu
def test_dump_outputs_is_the_last_timed_step(tmp_path, oracle):
    """bench.py --dump-outputs on the host-inclusive leg: warm-up max(--warmup, 3 x --host-threads) = 8 steps,
    then 2 regions x 3 timed steps, so the last timed step is step 13 and its queries are query set 13 % 8 = 5
    (seed 7 + 5).  The dump is that batch's result, bit for bit the oracle's."""
    import numpy as np
    from searchlite_amd import corpus
    out = tmp_path / "dump"
    r = _run(["--gpus", "1", "--config", "small", "--steps", "3", "--warmup", "8", "--regions", "2",
              "--host-threads", "1", "--no-cpu-baseline", "--check", "0", "--coalesce-threads", "0",
              "--dump-outputs", str(out)], timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = {n: np.load(out / f"{n}.npy") for n in ("doc_ids", "seg_ids", "scores", "counts", "query_rows")}
    seg = corpus.zipf_segment(100_000, 1 << 15, seed=42)
    offs, terms, w = corpus.zipf_queries(256, 3, seed=7 + 5, vocab=1 << 15)
    wd, _, wsc, wc = oracle.search_batch([seg], offs, terms, w, 11, strategy=oracle.BM25)
    assert np.array_equal(got["query_rows"], np.arange(256))
    assert np.array_equal(got["counts"], wc)
    for q in range(256):
        n = int(wc[q])
        assert np.array_equal(got["doc_ids"][q, :n], wd[q, :n]), q
        assert np.array_equal(got["scores"][q, :n], wsc[q, :n]), q

"""bench.py --dump-outputs: the writer on the host (no GPU), and a plain run's dump against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_writer(tmp_path):
    """small arrays whole (float64 where exact, else their bytes), a large one as a seeded byte sample plus
    chunk sums over every byte; the same arrays give the same files, and one changed byte shows in the sums"""
    import bench
    rng = np.random.default_rng(1)
    big = rng.integers(0, 1 << 63, (bench.DUMP_WHOLE // 8 + 1001,), dtype=np.uint64)
    arrays = {"bits": np.array([5, 1 << 40], np.uint64), "words": np.array([1 << 63, 3], np.uint64),
              "empty": np.zeros(0, np.uint64), "big": big}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, arrays)
    bench.dump_outputs(b, arrays)
    names = sorted(os.listdir(a))
    assert names == ["big_sample.npy", "big_sums.npy", "bits.npy", "empty.npy", "words.npy"]
    got = {n: np.load(os.path.join(a, n)) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert all(np.array_equal(v, np.load(os.path.join(b, n))) for n, v in got.items())
    assert got["bits.npy"].tolist() == [5.0, float(1 << 40)]
    assert np.array_equal(got["words.npy"], arrays["words"].view(np.uint8).astype(np.float32))
    by = big.view(np.uint8)
    assert got["big_sample.npy"].shape == (bench.DUMP_SAMPLE,) and got["big_sums.npy"].shape == (bench.DUMP_SUMS,)
    assert got["big_sums.npy"].sum() == by.sum(dtype=np.int64)
    assert set(np.unique(got["big_sample.npy"])) <= set(range(256))
    changed = big.copy()
    changed.view(np.uint8)[by.size // 3] ^= 1
    c = str(tmp_path / "c")
    bench.dump_outputs(c, {"big": changed})
    assert not np.array_equal(np.load(os.path.join(c, "big_sums.npy")), got["big_sums.npy"])
    assert sum(os.path.getsize(os.path.join(a, n)) for n in names) < bench.DUMP_LIMIT


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path, ctx, oracle):
    """a plain run (no --full) times exactly --steps steps, leaves the --full fields null, and its dump holds
    the last step's streams: those of the oracle for that step's image (steps + warmup = 3: the first of the
    two seeded images)"""
    import pybic
    rows, cols = 64, 4096
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", str(rows), "--cols", str(cols),
           "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 2 and j["ms_per_step"] > 0 and j["unit"] == "MPix/s" and j["full"] is False, j
    # value is the pixels of a step over ms_per_step (which the line rounds to 0.001 ms, value to 0.1)
    rel = 0.0005 / j["ms_per_step"] + 1e-3
    assert j["value"] == pytest.approx(rows * cols * 8 / (j["ms_per_step"] * 1e-3) / 1e6, rel=rel, abs=0.1), j
    for k in ("roofline", "predictor_pass", "kernels", "bit_exact_check", "cpu_baseline"):
        assert j[k] is None, (k, j[k])
    t = ctx.torch
    gen = t.Generator(device=ctx.dev)
    gen.manual_seed(0x5EED0000)
    gray = t.randint(0, 256, (rows, cols), dtype=t.uint8, device=ctx.dev, generator=gen).cpu().numpy()
    P = oracle.bitplanes(gray, 8)
    for coder, name in ((pybic.CODER_GOLOMB, "golomb"), (pybic.CODER_EG, "eg")):
        exp = [oracle.encode_plane(P[k], cols, 1, coder) for k in range(8)]
        bits = np.load(tmp_path / f"{name}_bits.npy")
        stream = np.load(tmp_path / f"{name}_stream.npy")
        assert bits.dtype == np.float64 and bits.tolist() == [float(e[0]) for e in exp]
        assert stream.dtype == np.float32
        assert stream.astype(np.uint8).tobytes() == b"".join(e[1].tobytes() for e in exp)

"""bench.py --dump-outputs DIR: the sampling and the files (CPU), a dump that fails keeps the line (CPU), and — on the GPU — that the dump is what the timed step computes,
pinned to the oracle from the seeded inputs, identical from run to run, whatever --steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from benchlib.common import DUMP_BUDGET_BYTES, dump_outputs, dumped_outputs_entry, sample_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_rows_is_fixed_sorted_and_within_budget():
    assert torch.equal(sample_rows(8, 16, 10**6), torch.arange(8))                 # fits: every row
    a, b = sample_rows(4096, 4 * 4096 + 4, 30 * 10**6), sample_rows(4096, 4 * 4096 + 4, 30 * 10**6)
    assert torch.equal(a, b) and a.numel() == 30 * 10**6 // (4 * 4096 + 4) and bool((a[1:] > a[:-1]).all()) and 0 <= int(a[0]) and int(a[-1]) < 4096
    assert sample_rows(10, 10**9, 100).numel() == 1                                # never empty


def test_dump_outputs_writes_float32_npy_below_the_budget(tmp_path):
    g = torch.Generator().manual_seed(3)
    arrays = {"y": torch.randn(4096, 4096, generator=g).to(torch.bfloat16), "x_codes": torch.randint(-128, 128, (4096, 4096), generator=g, dtype=torch.int8),
              "x_scale": torch.rand(4096, generator=g)}
    files = dump_outputs(str(tmp_path), arrays)
    assert set(files) == {"y.npy", "y_rows.npy", "x_codes.npy", "x_codes_rows.npy", "x_scale.npy"} == set(os.listdir(tmp_path))
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= DUMP_BUDGET_BYTES + 128 * len(files) < 64 * 10**6
    for name in ("y", "x_codes"):
        a, rows = np.load(tmp_path / f"{name}.npy"), np.load(tmp_path / f"{name}_rows.npy")
        assert a.dtype == np.float32 and rows.dtype == np.float32 and list(a.shape) == files[name + ".npy"] == [len(rows), 4096]
        assert np.array_equal(a, arrays[name].float().numpy()[rows.astype(np.int64)])          # exact: bf16 and int8 values are float32 values
    assert np.array_equal(np.load(tmp_path / "x_scale.npy"), arrays["x_scale"].numpy())
    assert np.array_equal(np.load(tmp_path / "y_rows.npy"), np.load(tmp_path / "x_codes_rows.npy"))
    # a small problem is written whole, and the row file of an earlier, larger dump in the same directory goes
    files = dump_outputs(str(tmp_path), {"y": arrays["y"][:64]})
    assert files == {"y.npy": [64, 4096]} and not os.path.exists(tmp_path / "y_rows.npy")
    assert np.array_equal(np.load(tmp_path / "y.npy"), arrays["y"][:64].float().numpy())


def test_arrays_of_the_same_rows_share_one_sample_whatever_their_widths(tmp_path):
    """N != K: row i of y.npy and of x_codes.npy is still the same token, and everything stays in the budget"""
    arrays = {"y": torch.ones(4096, 11008, dtype=torch.bfloat16), "x_codes": torch.ones(4096, 4096, dtype=torch.int8), "other": torch.ones(300, 8), "x_scale": torch.ones(4096)}
    files = dump_outputs(str(tmp_path), arrays)
    rows = np.load(tmp_path / "y_rows.npy")
    assert np.array_equal(rows, np.load(tmp_path / "x_codes_rows.npy")) and files["y.npy"] == [len(rows), 11008] and files["x_codes.npy"] == [len(rows), 4096]
    assert files["other.npy"] == [300, 8] and "other_rows.npy" not in files and len(rows) == (DUMP_BUDGET_BYTES - 4 * 4096 - 4 * 300 * 9) // (4 * (11008 + 4096) + 8)
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= DUMP_BUDGET_BYTES + 128 * len(files)
    with pytest.raises(ValueError, match="does not fit"):
        dump_outputs(str(tmp_path / "tiny"), {"y": torch.ones(64, 4096)}, budget_bytes=1000)


def test_a_dump_that_fails_keeps_the_line(tmp_path, capsys):
    blocker = tmp_path / "file"
    blocker.write_text("not a directory")
    e = dumped_outputs_entry(str(blocker / "dir"), {"y": torch.ones(4, 4)}, "what")
    assert "files" not in e and e["error"] and e["what"] == "what" and "--dump-outputs failed" in capsys.readouterr().err
    e = dumped_outputs_entry(str(tmp_path / "ok"), {"y": torch.ones(4, 4)}, "what")
    assert e["files"] == {"y.npy": [4, 4]} and "error" not in e and e["dtype"] == "float32"
    # and bench.py refuses a directory it cannot create BEFORE it measures anything
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", str(blocker / "dir")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr


def test_dump_outputs_is_refused_outside_the_headline_path():
    for extra in (["--workload", "mlp"], ["--mode", "tp"], ["--gpus", "2"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", "unused", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--dump-outputs" in r.stderr, (extra, r.stderr[-500:])


def _bench(tmp, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "3", "--repeats", "3", "--warmup-seconds", "0.2", "--no-cpu-baseline",
                        "--no-gpu-context", "--dump-outputs", str(tmp), *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dump_is_the_timed_steps_output_and_repeats_bit_for_bit(tmp_path):
    """two runs with different --steps: the line reports the steps asked for and the time of a block follows them; the files are identical; the codes and scales are the
    oracle's row quantisation of bench.py's seeded x, and y is QSPEC E1-E4 on them around the oracle's weight quantisation of the seeded weight (one row sample for all)."""
    from oracle import c_oracle as C
    from oracle import qspec_numpy as Q
    a, b = tmp_path / "a", tmp_path / "b"
    da, db = _bench(a, "--steps", "7"), _bench(b, "--steps", "60")
    assert da["steps"] == 7 and db["steps"] == 60 and da["verified"] is True and db["verified"] is True
    assert "x50 steps/replay" in db["config"]["launch"] and "x7 steps/replay" in da["config"]["launch"]
    # a block of 60 steps takes 60 / 7 times a block of 7 (ms_per_step = block / steps: were --steps not the number of steps run, the two would differ by that factor);
    # the short block carries more of the fixed cost of a replay, never less
    assert 0.9 * db["ms_per_step"] < da["ms_per_step"] < 1.6 * db["ms_per_step"], (da["ms_per_step"], db["ms_per_step"])
    assert abs(da["value"] - 2.0 * 4096**3 / (da["ms_per_step"] * 1e-3) / 1e12) < 0.02 * da["value"]
    files = da["dumped_outputs"]["files"]
    assert "error" not in da["dumped_outputs"] and "one sample" in da["dumped_outputs"]["what"]
    assert files == db["dumped_outputs"]["files"] and set(files) == set(os.listdir(a)) == set(os.listdir(b)) and {"y.npy", "x_codes.npy", "x_scale.npy"} <= set(files)
    assert sum(os.path.getsize(a / f) for f in files) < 64 * 10**6
    got = {f: np.load(a / f) for f in files}
    for f in files:
        assert got[f].dtype == np.float32 and list(got[f].shape) == files[f] and np.array_equal(got[f], np.load(b / f)), f
    rows = got["y_rows.npy"].astype(np.int64)
    assert np.array_equal(rows, got["x_codes_rows.npy"].astype(np.int64)) and np.isfinite(got["y.npy"]).all() and np.abs(got["y.npy"]).max() > 0
    bits = lambda t: t.view(torch.int16).numpy().view(np.uint16)       # noqa: E731
    # K1's dump against the oracle, from the seeds alone (bench.py: x from seed 1234 + rank, W from seed 4321)
    x = torch.randn(4096, 4096, generator=torch.Generator().manual_seed(1234)).to(torch.bfloat16)
    xq_o, xs_o = C.quant_rowwise(bits(x), 0)
    assert np.array_equal(got["x_scale.npy"], xs_o) and np.array_equal(got["x_codes.npy"], xq_o[rows].astype(np.float32))
    w = (torch.randn(4096, 4096, generator=torch.Generator().manual_seed(4321)) * 0.02).to(torch.bfloat16)
    wq, ws = C.quant_rowwise(bits(w), 0)
    acc = torch._int_mm(torch.from_numpy(xq_o[rows[:1024]]), torch.from_numpy(wq).t().contiguous()).numpy()
    want = Q.epilogue(acc, xs_o[rows[:1024]], ws, None, 0)
    assert np.array_equal(bits(torch.from_numpy(got["y.npy"][:1024]).to(torch.bfloat16)), want)

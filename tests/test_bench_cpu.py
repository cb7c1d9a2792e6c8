"""bench.py's host-side pieces (no GPU): the --dump-outputs writer and the argument surface."""
import numpy as np
import pytest
import torch


def test_dump_outputs_writes_float32_and_samples_large_arrays(tmp_path):
    import bench
    n = bench.DUMP_SAMPLE + 12_345
    big = (torch.arange(n, dtype=torch.float32) % 251).to(torch.bfloat16)  # exact in bf16
    small = torch.linspace(-1, 1, 77).view(7, 11)
    bench.dump_outputs(tmp_path / "a", {"big": big, "small": small, "loss": torch.tensor(2.5)})
    bench.dump_outputs(tmp_path / "b", {"big": big})
    got = {f.stem: np.load(f) for f in (tmp_path / "a").glob("*.npy")}
    assert sorted(got) == ["big", "loss", "small"]
    assert all(a.dtype == np.float32 and a.ndim == 1 for a in got.values())
    np.testing.assert_array_equal(got["small"], small.reshape(-1).numpy())
    np.testing.assert_array_equal(got["loss"], [2.5])
    # the sample: DUMP_SAMPLE entries, the same positions on every call, values from the array
    assert got["big"].shape == (bench.DUMP_SAMPLE,)
    np.testing.assert_array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))
    pos = np.sort(np.random.default_rng(1337).integers(0, n, size=bench.DUMP_SAMPLE))
    np.testing.assert_array_equal(got["big"], (pos % 251).astype(np.float32))
    # three sampled arrays stay under the 64 MB a dump may take
    assert 3 * bench.DUMP_SAMPLE * 4 <= 64e6


def test_bench_rejects_zero_steps(monkeypatch):
    import bench
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.main()

"""bench.py --dump-outputs on host tensors: the files it writes for the headline grid (names, float64 / float32 only, at
most 64 MB in all) and the seeded sample of grid points, which must not change from run to run."""
import os

import numpy as np
import torch


def _table(n):
    t = {key: torch.linspace(0.5, 1.5, n, dtype=torch.float64) for key in ("k", "w", "w_lo", "w_hi", "resid")}
    t["row"] = torch.arange(n, dtype=torch.int32) % 7
    t["flag"] = (torch.arange(n) % 2).to(torch.uint8)
    return t


def test_grid_sample_index_is_fixed():
    import bench
    n = bench.NK * bench.NW
    a, b = bench.grid_sample_index(n), bench.grid_sample_index(n)
    assert np.array_equal(a, b)
    assert len(a) == bench.DUMP_GRID_SAMPLE and np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < n
    assert np.array_equal(bench.grid_sample_index(1000), np.arange(1000))


def test_dump_outputs_headline_layout(tmp_path):
    import bench
    nbr = 40
    rows = torch.arange(0, 4 * bench.NK, 4)                      # global k-row of each local row (a strided tile)
    cols = bench.root_columns(_table(64), nbr, 1, rows)
    D = torch.arange(bench.NK * bench.NW, dtype=torch.float64).reshape(bench.NK, bench.NW)
    st = (torch.arange(bench.NK * bench.NW) % 4).to(torch.uint8).reshape(bench.NK, bench.NW)
    bench.dump_outputs(str(tmp_path), cols, (D, st))
    names = sorted(os.listdir(tmp_path))
    assert names == sorted([f"roots_{c}.npy" for c in ("k", "w", "w_lo", "w_hi", "resid", "flag", "unit", "row")]
                           + ["grid_sample_index.npy", "grid_D_sample.npy", "grid_status_sample.npy"])
    arrays = {n[:-4]: np.load(os.path.join(tmp_path, n)) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
    assert sum(os.path.getsize(os.path.join(tmp_path, n)) for n in names) <= 64 << 20
    assert all(arrays[f"roots_{c}"].shape == (nbr,) for c in ("k", "w", "resid", "flag", "unit", "row"))
    assert np.array_equal(arrays["roots_row"], 4.0 * (np.arange(nbr) % 7))
    assert np.all(arrays["roots_unit"] == 1.0)
    idx = arrays["grid_sample_index"].astype(np.int64)
    assert np.array_equal(idx, bench.grid_sample_index(D.numel()))
    assert np.array_equal(arrays["grid_D_sample"], idx.astype(np.float64))
    assert np.array_equal(arrays["grid_status_sample"], (idx % 4).astype(np.float32))

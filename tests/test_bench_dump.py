"""bench.py --dump-outputs: the arrays written are the dense outputs a caller of the timed path receives (no row padding,
no tile-slot padding), float32, and the same from run to run.  A stand-in workload of CPU tensors with padded rows and
64-pixel tile slots, exactly as bench.Workload lays them out, keeps this a CPU test."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _workload(n_tracks, T, H, tiles, seed=1):
    rs = np.random.default_rng(seed)
    spec = rs.standard_normal((n_tracks, T, H)).astype(np.float32)
    img = rs.integers(0, 1 << 16, (n_tracks, H, T)).astype(np.uint16)
    tile_px = sum(w * h for w, h in tiles)
    rgba = rs.integers(0, 256, (n_tracks, tile_px, 4)).astype(np.uint8)
    spec_p = np.full((n_tracks, T, H + 3), np.nan, np.float32)
    spec_p[:, :, :H] = spec
    img_p = np.zeros((n_tracks, H, T + 5), np.int16)
    img_p[:, :, :T] = img.view(np.int16)
    slots = [-(-(w * h) // 64) * 64 for w, h in tiles]
    rgba_p = np.full((n_tracks, sum(slots), 4), 7, np.uint8)
    off = px = 0
    for (w, h), s in zip(tiles, slots):
        rgba_p[:, off:off + w * h] = rgba[:, px:px + w * h]
        off, px = off + s, px + w * h
    wl = types.SimpleNamespace(
        n_tracks=n_tracks, T=T, H=H, tile_px=tile_px, geoms=[types.SimpleNamespace(width=w, height=h) for w, h in tiles],
        spec=torch.from_numpy(spec_p), img=torch.from_numpy(img_p), rgba=torch.from_numpy(rgba_p),
        minmax=torch.from_numpy(rs.standard_normal((n_tracks, 2)).astype(np.float32)), range_db=torch.tensor([-90.0, 10.0]))
    return wl, spec, img, rgba


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole_in_the_dense_layout(tmp_path):
    wl, spec, img, rgba = _workload(3, 37, 29, [(17, 13), (20, 13), (17, 5), (20, 5)])
    bench.dump_outputs(torch, wl, str(tmp_path))
    got = _load(tmp_path)
    assert sorted(got) == ["image_u16_sample", "minmax", "range_db", "spec_db_sample", "tiles_rgba_sample"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["spec_db_sample"], spec.reshape(-1))
    assert np.array_equal(got["image_u16_sample"], img.reshape(-1).astype(np.float32))
    assert np.array_equal(got["tiles_rgba_sample"], rgba.reshape(-1, 4).astype(np.float32))
    assert np.array_equal(got["minmax"], wl.minmax.numpy()) and got["range_db"].tolist() == [-90.0, 10.0]


def test_large_outputs_are_a_fixed_seeded_sample_within_the_budget(tmp_path):
    wl, spec, img, rgba = _workload(4, 900, 513, [(512, 512), (512, 1), (388, 512), (388, 1)])
    bench.dump_outputs(torch, wl, str(tmp_path / "a"))
    bench.dump_outputs(torch, wl, str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_MAX_BYTES
    rng = np.random.default_rng(bench.DUMP_SEED)   # the positions, drawn in the order dump_outputs draws them

    def pos(total):
        return np.sort(rng.choice(total, bench.DUMP_SAMPLE, replace=False))

    assert np.array_equal(a["spec_db_sample"], spec.reshape(-1)[pos(spec.size)])
    assert np.array_equal(a["image_u16_sample"], img.reshape(-1)[pos(img.size)].astype(np.float32))
    assert np.array_equal(a["tiles_rgba_sample"], rgba.reshape(-1, 4)[pos(rgba.shape[0] * rgba.shape[1])].astype(np.float32))

"""Mask morphology on the GPU (csrc/morph.hip; nn.MaskMorphology) against the checker of util_morph.py: integer equality, no tolerance.
1 x 7 is one row and one partial word, 5 x 64 one word per row (its own neighbour across the seam), 9 x 65 one valid bit in the last
word, 40 x 2048 more words than threads."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import nn as dnn  # noqa: E402
import util_morph as um  # noqa: E402

DEV = torch.device("cuda", 0)
MM = dnn.MaskMorphology
FILL = [("fill",)]
PROGRAMS = {"closing2": MM.closing(2), "fill": FILL, "opening3": MM.opening(3), "obr2": MM.opening_by_reconstruction(2),
            "chain": (MM.closing(1) + FILL + MM.opening_by_reconstruction(1), MM.closing(3) + FILL + MM.opening(2)), "empty": []}
SHAPES = [(1, 7), (5, 64), (9, 65), (33, 130), (40, 2048)]


def _pair(steps):
    return steps if isinstance(steps, tuple) else (steps, steps)


@functools.lru_cache(maxsize=None)
def _case(shape, nb, seed, program, wrap):
    mask = um.noise_mask(*shape, nb, seed)
    return mask, um.morph(mask, *_pair(PROGRAMS[program]), wrap)


def _check(mask, ref, steps, wrap, dtype=torch.uint8, n_valid=None):
    nb, H, W = mask.shape
    nv = nb if n_valid is None else n_valid
    mm = MM(nb, H, W, steps, wrap=bool(wrap), device=DEV)
    guards = (mm._out, mm._counts, mm._rounds, mm._converged)
    for t in guards:
        t.fill_(0x5A)
    mm(torch.from_numpy(mask).to(DEV).to(dtype), n_valid=nv)
    torch.cuda.synchronize()
    out, counts, ran = ref
    got = mm.mask_buffer.cpu().numpy()
    bad = np.argwhere(got[:nv] != out[:nv])
    assert len(bad) == 0, f"{len(bad)} pixels differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} vs {out[tuple(bad[0])]}"
    assert [[list(c.values()) for c in f] for f in mm.counts()] == counts[:nv].tolist() and list(mm.counts()[0][0]) == list(dnn.MORPH_COUNTS)
    assert ((mm.rounds() > 0) == ran[None]).all() and (mm.converged() == 1).all()
    for t in guards:                                    # the padding samples keep their guard bytes
        assert bool((t[nv:] == 0x5A).all())
    return mm


@pytest.mark.parametrize("wrap", [0, 1])
@pytest.mark.parametrize("program", list(PROGRAMS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_masks_and_counts_match_the_checker(shape, program, wrap):
    mask, ref = _case(shape, 2, 7, program, wrap)
    _check(mask, ref, PROGRAMS[program], wrap)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_wide_masks_padding_samples_and_other_values(dtype):
    """three frames, two of them valid; 3 and 255 are copied verbatim and belong to neither plane"""
    mask = um.noise_mask(33, 130, 3, seed=11)
    mask[:, 4:9, 20:40][mask[:, 4:9, 20:40] == 0] = 3
    mask[:, 20:24, 60:90][mask[:, 20:24, 60:90] == 1] = 255
    steps = PROGRAMS["chain"]
    ref = um.morph(mask, *steps, 1)
    assert (ref[0] == 3).any() and (ref[0] == 255).any()
    _check(mask, ref, steps, 1, dtype=dtype, n_valid=2)
    _check(mask, ref, steps, 1, n_valid=2)              # ... and as bytes: 130 is no multiple of 16, the pixel-by-pixel pass


@pytest.mark.parametrize("wrap", [0, 1])
@pytest.mark.parametrize("program", ["fill", "obr2"])
def test_spiral_corridor_needs_many_rounds(program, wrap):
    """a flood that advances one pixel a round, or stops at the first quiet thread, fails here"""
    mask = um.spiral_mask(33, 130)
    ref = um.morph(mask, *_pair(PROGRAMS[program]), wrap)
    assert np.array_equal(ref[0], mask)                 # the corridor is no hole; the line comes back from the block's seed
    _check(mask, ref, PROGRAMS[program], wrap)


@pytest.mark.parametrize("shape", [(768, 1152), (21, 32800)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_large_planes(shape):
    """768 x 1152: the workload's plane, a thread's run is 14 rows of one column.  21 x 32800: 513 columns of words, which no cut of
    whole columns spreads over 1024 threads, so the runs pass from the foot of a column to the head of the next"""
    mask, ref = _case(shape, 1, 5, "chain", 1)
    _check(mask, ref, PROGRAMS["chain"], 1)


def test_predict_cli_with_morphology(tmp_path):
    import json, os, subprocess, sys  # noqa: E401
    from mlperf_deepcam_amd import h5lite
    import util_val
    if not h5lite.available():
        pytest.skip("no HDF5 C library in this image")
    H, W = util_val.H, util_val.W
    root, stats = str(tmp_path / "unlabelled"), str(tmp_path / "stats.h5")
    os.makedirs(root)
    rs, names = np.random.RandomState(12), [f"data-{i:02d}.h5" for i in range(2)]
    fields = [(rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in range(2)]
    for name, d in zip(names, fields):
        with h5lite.File(os.path.join(root, name), "w") as f:
            f.write("climate/data", d)
    with h5lite.File(stats, "w") as f:
        f.write("climate/minval", np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
        f.write("climate/maxval", np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
    ckpt, out = str(tmp_path / "model_step_7.cpt"), str(tmp_path / "out")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)
    cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--output_dir",
           out, "--batch_size", "2", "--dtype", "fp32", "--height", str(H), "--width", str(W), "--max_inter_threads", "2", "--events",
           "--morph_close", "1", "2", "--morph_fill", "--morph_open", "0", "1", "--morph_open_reconstruct"]
    r = subprocess.run(cmd, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    steps = (MM.closing(1) + FILL, MM.closing(2) + FILL + MM.opening_by_reconstruction(1))
    total = np.zeros((2, 4), np.int64)
    for name in names:
        with h5lite.File(os.path.join(out, name)) as f:
            p, pm, mc, ev = (f.read(k) for k in ("prediction", "prediction_morph", "morph_counts", "events"))
        ref_out, ref_counts, _ = um.morph(p[None], *steps, 1)
        assert pm.dtype == np.uint8 and np.array_equal(pm, ref_out[0]) and np.array_equal(mc, ref_counts[0])
        assert [int(ev[ev[:, 1] == k, 2].sum()) for k in (1, 2)] == [int((pm == k).sum()) for k in (1, 2)]     # the catalogue took the cleaned mask
        total += mc
    sm = json.load(open(os.path.join(out, "summary.json")))["morphology"]
    assert sm["steps"] == [[list(s) for s in st] for st in steps]
    assert [[c[k] for k in dnn.MORPH_COUNTS] for c in sm["classes"]] == total.tolist()

"""Train-time augmentation without a GPU (data.Augment, data.to_source, train.py --augment_*): the draw rule pinned and its properties, the
sharding invariance, the coordinate round trip, the checker of tests/util_augment.py against plain numpy, the refusals and the parser."""
import numpy as np
import pytest
import torch

from mlperf_deepcam_amd import data as ddata
from mlperf_deepcam_amd import train
import util_augment as ua
import util_ensemble as ue

NAMES = [f"data-synthetic-{i:06d}.h5" for i in range(4096)]


def _table(aug, epoch, W, names=NAMES):
    return np.asarray([aug.draw(epoch, n, W) for n in names], np.int64)


def test_draw_rule_is_pinned():
    """default_rng([seed, epoch, crc32(basename)]), integers(0, W) then integers(0, 2): other values mean another rule"""
    aug = ddata.Augment(roll=True, flip_lat=True, seed=0)
    assert [aug.draw(0, f"data-synthetic-00000{i}.h5", 1152) for i in range(4)] == [(524, 0), (147, 0), (901, 0), (575, 1)]
    assert aug.draw(0, "/x/y/data-synthetic-000000.h5", 1152) == (524, 0)                # the basename only
    for i in range(4):                                                                   # the checker states the same rule
        assert ua.draw(0, 0, NAMES[i], 1152) == aug.draw(0, NAMES[i], 1152)
    assert all(type(v) is int for v in aug.draw(0, NAMES[0], 1152))


def test_draw_rule_properties():
    aug = ddata.Augment(roll=True, flip_lat=True, seed=0)
    for W in (12, 64, 1152):
        t = _table(aug, 0, W)
        assert t[:, 0].min() >= 0 and t[:, 0].max() < W and set(t[:, 1].tolist()) == {0, 1}
        if W <= 64:
            assert set(t[:, 0].tolist()) == set(range(W))                                # every column occurs
        else:
            # 4096 uniform draws miss a given column with probability (1 - 1/1152)^4096 = 0.0286: 1119 distinct columns expected, with a
            # standard deviation below 6
            assert len(set(t[:, 0].tolist())) > 1080 and t[:, 0].min() < 8 and t[:, 0].max() >= W - 8
    t = _table(aug, 0, 1152)
    residues = np.bincount(t[:, 0] % 4, minlength=4)
    print("roll mod 4:", residues.tolist(), "flips:", t[:, 1].mean())                    # 1009 / 998 / 1067 / 1022, 0.5088
    assert all(900 <= int(c) <= 1150 for c in residues)
    assert 0.45 <= t[:, 1].mean() <= 0.55
    same = lambda a, b: int((a == b).all(axis=1).sum())  # noqa: E731
    e1, s1 = same(t, _table(aug, 1, 1152)), same(t, _table(ddata.Augment(roll=True, flip_lat=True, seed=1), 0, 1152))
    print("agreeing with (epoch 0, seed 0): epoch 1", e1, "seed 1", s1)                  # 2 and 2
    assert e1 < 16 and s1 < 16
    # switching one kind off does not move the other's draws
    only_flip = _table(ddata.Augment(flip_lat=True, seed=0), 0, 1152)
    only_roll = _table(ddata.Augment(roll=True, seed=0), 0, 1152)
    assert (only_flip[:, 0] == 0).all() and (only_flip[:, 1] == t[:, 1]).all()
    assert (only_roll[:, 1] == 0).all() and (only_roll[:, 0] == t[:, 0]).all()
    assert (ua.draws(0, 0, NAMES, 1152, roll=False) == only_flip).all() and (ua.draws(0, 0, NAMES, 1152, flip_lat=False) == only_roll).all()


def test_views_do_not_depend_on_the_sharding():
    """file -> view over one epoch: one process that stands for four ranks, and four processes of one rank each"""
    aug = ddata.Augment(roll=True, flip_lat=True, seed=3)
    names, B, W, epoch = NAMES[:70], 2, 1152, 5

    def epoch_map(comm_size, K):
        out = {}
        for rank in range(comm_size):
            files, _ = ddata.shard_files_virtual(names, comm_size, rank, K, B, False, True)
            for s in range(len(files) // (K * B)):                                       # the batches InputPipeline stages, slot by slot
                batch = files[s * K * B:(s + 1) * K * B]
                for f, v in zip(batch, ua.slot_views(3, epoch, batch, K * B, W)):
                    assert f not in out and tuple(v) == aug.draw(epoch, f, W)
                    out[f] = tuple(v)
        return out
    one, four = epoch_map(1, 4), epoch_map(4, 1)
    assert len(one) == 64 and one == four


def test_to_source_inverts_to_view():
    rs = np.random.RandomState(5)
    B, H, W = 5, 6, 10
    m = rs.randint(-2 ** 40, 2 ** 40, size=(B, H, W)).astype(np.int64)
    views = np.asarray([(0, 0), (W - 1, 1), (3, 0), (0, 1), (7, 1)], np.int32)
    viewed = np.stack([ue.to_view(m[n], int(r), bool(f)) for n, (r, f) in enumerate(views)])
    assert not (viewed == m)[1:].all()
    back = ddata.to_source(torch.from_numpy(np.ascontiguousarray(viewed)), views)
    assert back.dtype == torch.int64 and (back.numpy() == m).all()
    for n, (r, f) in enumerate(views):                                                   # and it is util_ensemble's to_source, per sample
        assert (back[n].numpy() == ue.to_source(viewed[n], int(r), bool(f))).all()
    assert (ddata.to_source(torch.from_numpy(np.ascontiguousarray(viewed)).to(torch.uint8), views).numpy() == m.astype(np.uint8)).all()
    with pytest.raises(ValueError):
        ddata.to_source(torch.zeros(B, H, W), views)
    with pytest.raises(ValueError):
        ddata.to_source(torch.zeros(B, H, W, dtype=torch.int64), views[:-1])


def test_checker_views_are_numpy_roll_and_flip():
    rs = np.random.RandomState(6)
    B, H, W, cfile = 3, 5, 12, 16
    lab = rs.randint(0, 3, size=(B, H, W)).astype(np.int64)
    views = [(0, 0), (W - 1, 1), (5, 0)]
    got = ua.viewed_labels(lab, views)
    for n, (r, f) in enumerate(views):
        assert (got[n] == np.roll(np.flip(lab[n], 0) if f else lab[n], -r, axis=1)).all()
        for h in range(H):
            for w in range(W):
                assert got[n, h, w] == lab[n][ue.source_of(h, w, H, W, r, f)]
    x = rs.rand(B, H, W, cfile).astype(np.float32) * 100 - 30
    channels = [1, 2, 4, 7, 8, 11, 13, 15]
    sign = np.where(np.isin(channels, [4, 13]), -1.0, 1.0)
    shift, scale = rs.rand(8).astype(np.float32), rs.rand(8).astype(np.float32) + 0.5
    out = ua.viewed_batch(x, channels, sign, shift, scale, views)
    assert out.shape == (B, H, W, 8)
    for n, (r, f) in enumerate(views):
        moved = np.roll(np.flip(x[n], 0) if f else x[n], -r, axis=1)[..., channels].astype(np.float64)
        want = scale.astype(np.float64) * ((sign if f else 1.0) * moved - shift.astype(np.float64))
        assert (out[n] == want).all()
    assert (ua.slot_views(0, 0, NAMES[:2], 4, 64)[1:] == ua.draws(0, 0, [NAMES[1]] * 3, 64)).all()


def test_refusals():
    with pytest.raises(ValueError):
        ddata.Augment()
    with pytest.raises(ValueError):
        ddata.Augment(roll=True, negate=(2, 4))
    a = ddata.Augment(flip_lat=True, negate=(2, 4), seed=7)
    assert (a.roll, a.flip_lat, a.negate, a.seed) == (False, True, [2, 4], 7)


def test_parser():
    a = train.build_parser().parse_args([])
    assert (a.augment_roll, a.augment_flip_lat, a.augment_negate, a.augment_seed) == (False, False, [], 0)
    a = train.build_parser().parse_args(["--augment_roll", "--augment_flip_lat", "--augment_negate", "2", "4", "--augment_seed", "5"])
    assert (a.augment_roll, a.augment_flip_lat, a.augment_negate, a.augment_seed) == (True, True, [2, 4], 5)
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--augment_negate", "2", "4"])
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--augment_roll", "--augment_negate", "2", "4"])
    # run_scripts/run_training_dgx2.sh:51-70 as tests/test_train_cli_cpu.py hands it over: the same values as ever
    argv = ["--wireup_method", "nccl-openmpi", "--run_tag", "deepcam_prediction_run1", "--data_dir_prefix", "/data", "--output_dir", "/data/runs/x",
            "--max_inter_threads", "2", "--model_prefix", "classifier", "--optimizer", "LAMB", "--start_lr", "1e-3",
            "--lr_schedule", 'type="multistep",milestones="15000 25000",decay_rate="0.1"', "--lr_warmup_steps", "0", "--lr_warmup_factor", "1.",
            "--weight_decay", "1e-2", "--validation_frequency", "200", "--training_visualization_frequency", "200",
            "--validation_visualization_frequency", "40", "--max_validation_steps", "50", "--logging_frequency", "0", "--save_frequency", "400",
            "--max_epochs", "200", "--amp_opt_level", "O1", "--local_batch_size", "2"]
    a = train.build_parser().parse_args(argv)
    assert a.lr_schedule == {"type": "multistep", "milestones": "15000 25000", "decay_rate": "0.1"}
    assert (a.optimizer, a.weight_decay, a.local_batch_size, a.amp_opt_level, a.logging_frequency) == ("LAMB", 1e-2, 2, "O1", 0)
    assert (a.max_epochs, a.save_frequency, a.validation_frequency, a.max_validation_steps, a.run_tag) == (200, 400, 200, 50, "deepcam_prediction_run1")
    assert (a.augment_roll, a.augment_flip_lat, a.augment_negate, a.augment_seed) == (False, False, [], 0)

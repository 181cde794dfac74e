"""Virtual ranks, host side (no GPU): the interleaved sample assignment of the driver and TrainStep's scaling / refusal logic."""
import pytest
import torch

from mlperf_deepcam_amd import data as ddata
from mlperf_deepcam_amd import dist as ddist
from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
from mlperf_deepcam_amd import spec

FILES = [f"data-{i:03d}.h5" for i in range(37)]


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("B", [1, 2])
def test_shard_interleave_reproduces_the_larger_job(R, K, B):
    """Process r of R with K virtual ranks: step s, micro-batch v holds the samples global rank r*K+v reads in step s of an R*K-rank job."""
    for r in range(R):
        mine, gsize = ddata.shard_files_virtual(FILES, R, r, K, B, False, True)
        shards = [ddata.shard_files(FILES, R * K, r * K + v, False, True) for v in range(K)]
        assert gsize == shards[0][1] == R * K * (37 // (R * K))
        steps = len(shards[0][0]) // B
        assert steps >= 1
        if K == 1:
            assert mine == shards[0][0]                   # today's list, ragged tail included (the loader drops it)
        else:
            assert len(mine) == steps * K * B
        for s in range(steps):
            for v in range(K):
                assert mine[(s * K + v) * B:(s * K + v + 1) * B] == shards[v][0][s * B:(s + 1) * B], (r, s, v)
    # no sample is read by two processes
    every = [f for r in range(R) for f in ddata.shard_files_virtual(FILES, R, r, K, B, False, True)[0]]
    assert len(set(every)) == len(every)


def test_synthetic_dataset_takes_the_interleaved_shard():
    ds = ddata.SyntheticHWC(16, 64, 96, shuffle=True, comm_size=1, comm_rank=0, virtual_ranks=2, batch_size=2)
    want, gsize = ddata.shard_files_virtual([f"data-synthetic-{i:06d}.h5" for i in range(16)], 1, 0, 2, 2, False, True)
    assert ds.files == want and ds.global_size == gsize == 16 and len(ds) == 16


class _Engine:
    """What TrainStep's host logic needs from an engine (host arenas, as the reducer's CPU tests use)."""

    def __init__(self):
        self.layout = spec.Layout()
        self.device = torch.device("cpu")
        self.B, self.H, self.W, self.n_input = 2, 64, 96, 16
        self.grads = torch.zeros(self.layout.n_params)
        self.grad_acc = None
        self.on_grad_ready = None

    def enable_grad_accumulation(self):
        if self.grad_acc is None:
            self.grad_acc = torch.empty_like(self.grads)
        return self.grad_acc


class _Net:
    act_dtype, n_input = torch.float32, 16

    def __init__(self):
        self.engine = _Engine()

    def engine_for(self, shape):
        return self.engine


class _Opt:
    grad_scale, grad_arena = 1.0, None

    def use_gradients(self, arena):
        self.grad_arena = arena


class _Reducer(ddist.GradReducer):
    def __init__(self, eng, world, collective="torch"):
        super().__init__(eng, 1, collective=collective, comm=object())
        self.world = world


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_gradient_scale_is_one_over_ranks(K):
    net, opt = _Net(), _Opt()
    step = dnn.TrainStep(net, opt, dnn.class_weights(), 2, 64, 96, virtual_ranks=K)
    assert opt.grad_scale == 1.0 / K
    if K == 1:
        assert net.engine.grad_acc is None and opt.grad_arena is None and net.engine.on_grad_ready is None
    else:
        assert opt.grad_arena is net.engine.grad_acc and net.engine.grad_acc is not None
        assert step._reducer.acc is net.engine.grad_acc and net.engine.on_grad_ready == step._reducer.ready
    for world in (2, 8):
        red = _Reducer(net.engine, world)
        step.attach_reducer(red)
        assert opt.grad_scale == 1.0 / (K * world) and red.averaging_in_optimizer
        assert net.engine.on_grad_ready == red.ready
        assert red.acc is (net.engine.grad_acc if K > 1 else None)


def test_recording_a_virtual_rank_step_with_a_reducer_is_refused():
    net, opt = _Net(), _Opt()
    step = dnn.TrainStep(net, opt, dnn.class_weights(), 2, 64, 96, virtual_ranks=2)
    step.attach_reducer(_Reducer(net.engine, 2, collective="library"))
    with pytest.raises(L.DeepcamHipError, match="virtual ranks with a gradient reducer attached runs eagerly only"):
        step.enable_program()
    with pytest.raises(L.DeepcamHipError, match="virtual_ranks must be at least 1"):
        dnn.TrainStep(net, opt, dnn.class_weights(), 2, 64, 96, virtual_ranks=0)


def test_driver_has_the_flag():
    from mlperf_deepcam_amd import train
    p = train.build_parser()
    assert p.parse_args([]).virtual_ranks == 1 and p.parse_args(["--virtual_ranks", "8"]).virtual_ranks == 8

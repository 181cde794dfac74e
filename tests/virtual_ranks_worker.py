"""Worker for tests/test_virtual_ranks_gpu.py: 2 ranks (gloo, both on cuda:0) run three LAMB steps of the fused TrainStep with the gradient
reducer attached, each on its own batches (batch(rank, step)); rank 0 writes the weights, its BatchNorm buffers and every step's two rank
losses to the file named on the command line.  The test runs the same data as ONE process with two virtual ranks and compares."""
import os, sys, torch, torch.distributed as dist
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from mlperf_deepcam_amd import dist as comm, nn as dnn
from mlperf_deepcam_amd.dist import DistributedDataParallel as DDP
from util_inputs import make_inputs

B, H, W, STEPS, OPT = 2, 64, 96, 3, "LAMB"


def batch(rank, step):
    return make_inputs(B, H, W, seed=1234 + rank + 10 * step)


def main():
    out_path = sys.argv[1]
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[sys.argv[2]]
    comm.init("env", backend="gloo")
    rank, world = comm.get_rank(), comm.get_size()
    torch.cuda.set_device(0); dev = torch.device("cuda", 0); cw = dnn.class_weights()
    net = dnn.DeepLabv3_plus(n_input=16, n_classes=3, os=16, pretrained=False, rank=rank, _print=False, dtype=dtype, seed=333)
    net.materialize(B, H, W)
    opt = dnn.make_optimizer(OPT, net, 1e-3, 1e-8, 1e-2)
    ddp = DDP(net)
    ts = dnn.TrainStep(net, opt, cw, B, H, W, with_metrics=True)
    ts.attach_reducer(ddp.reducer)
    losses = []
    for step in range(STEPS):
        x, y = batch(rank, step)
        ts(x.to(dev), y.to(dev))
        torch.cuda.synchronize()
        mine = torch.tensor([ts.loss()], dtype=torch.float64)
        both = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(both, mine)
        losses.append([float(t) for t in both])
    if rank == 0:
        torch.save({"params": net.engine.params.cpu(), "buffers": net.engine.buffers.cpu(), "nbt": net.engine.nbt.cpu(), "losses": losses}, out_path)
        print("VR_WORKER ok", flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""MI355X-native DeepCAM train step: host side (Python) over libdeepcam_hip.so (hand-written gfx950 kernels).

Import as ``mlperf_deepcam_amd``.  Layout:
  csrc/            HIP kernels + the C ABI (include/deepcam_hip.h)
  lib.py           ctypes binding of the C ABI (fails loudly if the library is missing)
  ops.py           the step's operators registered with torch's dispatcher (torch.ops.deepcam.*)
  spec.py          layer table of DeepLabV3+/Xception and parameter-arena layout
  engine.py        explicit forward / backward program over preallocated NHWC buffers
  nn.py            reference-compatible call surface: DeepLabv3_plus, fp_loss, compute_score, optimizers, schedules, TrainStep,
                   ValStep, Predictor; re-exports the analysis modules' names
  events.py        event catalogue, matching, per-event fields, shapes, filter, tracks and track life cycles
  render.py        frame renderer: the visualiser's picture drawn on the device
  climate.py       climatology maps over time and storm-centred composites
  skills.py        verification skills: neighbourhood, distance-map, displacement, scale-separation, probabilistic
  decide.py        decision rule (probability thresholds with hysteresis) and view ensemble
  _args.py         argument checks the analysis modules share
  dist.py          comm wire-up + RCCL gradient all-reduce overlapped with backward
  data.py          input pipeline: files -> pinned host buffers -> HBM (copy stream) -> normalised NHWC activations
  h5lite.py        minimal HDF5 access through the HDF5 C library (ctypes), for images without h5py
  png.py           PNG writer and reader (zlib and struct)
  prep.py          dataset statistics file and train / validation / test split
  train.py         train_hdf5_ddp.py-compatible driver (CLI, checkpoints, MLLOG lines)
  predict.py       inference driver: checkpoint + unlabelled files -> one mask file per input file
  profile.py       phase-bracketed profiling driver (profile_hdf5_ddp.py's counterpart)
"""
__version__ = "0.1.0"

"""Static instruction counts of dwp_kernel's tile loop per instantiation, from the compiler's assembly of csrc/dwpipe.hip:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -I mlperf-deepcam_amd/csrc mlperf-deepcam_amd/csrc/dwpipe.hip -o dwpipe.s
    python scripts/dwp_isa_count.py dwpipe.s [dwpipe_parent.s]

The tile loop is the loop that holds the per-tile s_barrier.  Counts are per wave and tile, over every block of the loop (the arms of
the vmcnt ladder are all counted: a handful of scalar instructions more than one trip executes).  With two files: the second one's
counts beside the first's."""
import collections, re, sys

MODES = {1: "FLIP", 2: "STATS", 4: "WGRAD", 8: "ADD", 16: "XFORM", 32: "RES", 64: "MASK"}


def mode_name(m):
    return "|".join(n for b, n in MODES.items() if m & b) or "fwd"


def classify(op):
    if op.startswith("v_pk_fma"): return "v_pk_fma"
    if op.startswith("v_fma") or op.startswith("v_fmac"): return "v_fma"
    if op.startswith("v_cvt_pk_bf16"): return "cvt_pk"
    if op.startswith("v_"): return "v_other"
    if op.startswith("ds_read2") or op.startswith("ds_read_b128"): return "ds_read2"
    if op.startswith("ds_"): return "ds_other"
    if op.startswith("buffer_load"): return "lds_dma"
    if op.startswith("global_store") or op.startswith("buffer_store"): return "store"
    if op.startswith("s_waitcnt"): return "waitcnt"
    if op.startswith("s_"): return "scalar"
    return "other"


def count(path):
    out = {}
    name, blocks, cur, regs = None, None, None, None
    for line in open(path):
        m = re.match(r"^(_ZN\S*dwp_kernelILi(\d+)ELi(\d+)E\S*):", line)
        if m:
            name, blocks, cur = (int(m.group(2)), int(m.group(3))), collections.OrderedDict(), None
            continue
        if name is None:
            continue
        m = re.match(r"^(\.LBB\d+_\d+):(.*)", line)
        if m:
            h = re.search(r"Header=(BB\d+_\d+)|This Inner Loop Header", m.group(2))
            loop = None
            if h:
                loop = ".L" + h.group(1) if h.group(1) else m.group(1)
            cur = (m.group(1), loop)
            blocks[cur] = []
            continue
        m = re.match(r"^; NumVgprs: (\d+)", line)
        if m: regs = int(m.group(1))
        m = re.match(r"^; ScratchSize: (\d+)", line)
        if m:
            # the loop whose blocks hold a barrier
            loops = collections.defaultdict(list)
            for (lab, loop), ins in blocks.items():
                if loop: loops[loop].extend(ins)
            tile = [ins for ins in loops.values() if "s_barrier" in ins]
            c = collections.Counter(classify(op) for op in tile[0]) if tile else collections.Counter()
            c["vgprs"], c["scratch"] = regs, int(m.group(1))
            c["vector"] = c["v_pk_fma"] + c["v_fma"] + c["cvt_pk"] + c["v_other"]
            out[name] = c
            name = None
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]+)", line)
        if m and cur is not None and not line.lstrip().startswith("."):
            blocks[cur].append(m.group(1))
    return out


COLS = ["vector", "v_pk_fma", "v_fma", "cvt_pk", "v_other", "scalar", "waitcnt", "ds_read2", "ds_other", "lds_dma", "store", "vgprs", "scratch"]
tabs = [count(p) for p in sys.argv[1:3]]
print(f"{'dil':>3} {'mode':>4} {'riders':28s}" + "".join(f"{c:>10s}" for c in COLS))
for key in sorted(tabs[0]):
    for i, t in enumerate(tabs):
        if key in t:
            tag = mode_name(key[1]) + (" (2nd file)" if i else "")
            print(f"{key[0]:>3} {key[1]:>4} {tag:28s}" + "".join(f"{t[key][c]:>10d}" for c in COLS))

"""Decision rule (DecisionRule: a mask from the logits by probability thresholds with hysteresis) and view ensemble (view_input,
ViewEnsemble: the logits of rolled and mirrored views pooled), on the device."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import lib as L
from ._args import _n_valid, _ratio, check_tensor, device_of
from .skills import PROB_MAX_BATCH, PROB_MAX_BINS, PROB_MAX_PIXELS, PROB_ONE

DECISION_NEVER = PROB_ONE + 1                     # a threshold no q reaches
DECISION_COUNTS = ("class1_candidate_pixels", "class1_seed_pixels", "class1_kept_pixels", "class1_candidate_events", "class1_kept_events",
                   "class2_candidate_pixels", "class2_seed_pixels", "class2_kept_pixels", "class2_candidate_events", "class2_kept_events",
                   "nonfinite_pixels", "conflict_pixels")


def decision_q(p) -> int:
    """The threshold on q = rint(softmax * 65536) for the probability p: ceil(p * 65536) clamped to [0, 65537], so that q >= decision_q(p)
    iff q / 65536 >= p.  p > 1 gives 65537: never."""
    p = float(p)
    if math.isnan(p):
        raise L.DeepcamHipError("decision_q: the probability is NaN")
    if p > 1.0:
        return DECISION_NEVER
    return max(0, int(math.ceil(p * PROB_ONE)))


def decision_q_from_bin(k: int, bins: int) -> int:
    """The threshold on q that reproduces ProbabilitySkill's forecast "class c at threshold k / bins", min(bins - 1, (q * bins) >> 16) >= k:
    ceil(k * 65536 / bins) for k < bins, 65537 (never) for k == bins."""
    k, bins = int(k), int(bins)
    if not 1 <= bins <= PROB_MAX_BINS or not 0 <= k <= bins:
        raise L.DeepcamHipError(f"decision_q_from_bin: bins must lie in [1, {PROB_MAX_BINS}] and k in [0, bins], got k = {k}, bins = {bins}")
    return DECISION_NEVER if k == bins else -((-k * PROB_ONE) // bins)


class DecisionRule:
    """A mask from the classifier's fp32 logits by per-class probability thresholds with hysteresis, on the device (dc_logits_decide,
    dc_mask_components, dc_hysteresis_select; csrc/decide.hip) -- instead of the argmax, which the training's class weights bias on purpose.
    With q_c = rint(softmax_c * 65536), ProbabilitySkill's integer: class c in (1, 2) qualifies at a pixel iff q_c >= low[c]; the candidate
    class is the qualifying one, of two the one with the larger q (class 1 on equal q), else 0; a candidate pixel with q_c >= high[c] is a
    seed; the mask keeps the connected components of the candidates (one class, `connectivity` 4 or 8, periodic columns with `wrap`) that
    hold a seed.  A pixel with a logit that is not finite is background.  high=None, or high == low: plain thresholding, no component pass.
    low and high are pairs (class 1, class 2): a float is a probability (decision_q), an int is q itself, in [0, 65537]; 65537 is never.
    Memory with hysteresis: 4 * B * H * W bytes of planes (candidates, seeds, flags, mask) plus 4 * B * H * W bytes of labels plus the
    workspace of dc_mask_components; without: one plane of B * H * W bytes.  A call launches on the current stream and does not
    synchronise; the mask is whatever consumes a mask takes (EventFilter, EventCatalog, EventMatcher, FractionsSkill, ...)."""

    def __init__(self, batch: int, height: int, width: int, low=(0.5, 0.5), high=None, connectivity: int = 8, wrap: bool = True, device=None):
        if batch < 1 or batch > PROB_MAX_BATCH or height < 1 or width < 1 or height * width > PROB_MAX_PIXELS:
            raise L.DeepcamHipError(f"DecisionRule: batch must lie in [1, {PROB_MAX_BATCH}], height and width be positive and height * width at most 2^30")
        if connectivity not in (4, 8):
            raise L.DeepcamHipError(f"DecisionRule: connectivity must be 4 or 8, got {connectivity}")
        self.low = self._pair(low, "low")
        self.high = self.low if high is None else self._pair(high, "high")
        if any(h < l for l, h in zip(self.low, self.high)):
            raise L.DeepcamHipError(f"DecisionRule: a high threshold must not be below its low threshold, got low = {self.low}, high = {self.high} (q)")
        self.hysteresis = self.high != self.low
        self.B, self.H, self.W, self.connectivity, self.wrap = batch, height, width, connectivity, bool(wrap)
        dev = torch.device(device_of(device))
        self._counts = torch.zeros((batch, len(DECISION_COUNTS)), dtype=torch.int64, device=dev)
        dev = self.device = self._counts.device
        plane = lambda: torch.zeros((batch, height, width), dtype=torch.uint8, device=dev)  # noqa: E731
        self._cand = plane()
        self._seed = self._flags = self._out = self._labels = self._ws = None
        if self.hysteresis:
            self._seed, self._out = plane(), plane()
            self._flags = torch.zeros(max(L.load().dc_decide_workspace(batch, height, width), 256), dtype=torch.uint8, device=dev)
            self._labels = torch.zeros((batch, height, width), dtype=torch.int32, device=dev)
            self._ws = torch.empty(max(L.load().dc_mask_components_workspace(batch, height, width), 256), dtype=torch.uint8, device=dev)
        self._last_valid = 0

    @staticmethod
    def _pair(v, name):
        if not isinstance(v, (tuple, list, np.ndarray)) or len(v) != 2:
            raise L.DeepcamHipError(f"DecisionRule: {name} takes two values (class 1, class 2), got {v!r}")
        out = []
        for x in v:
            if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
                raise L.DeepcamHipError(f"DecisionRule: {name} takes probabilities (float) or q (int), got {x!r}")
            q = int(x) if isinstance(x, (int, np.integer)) else decision_q(x)
            if not 0 <= q <= DECISION_NEVER:
                raise L.DeepcamHipError(f"DecisionRule: a threshold q must lie in [0, {DECISION_NEVER}], got {name} = {x!r}")
            out.append(q)
        return tuple(out)

    @staticmethod
    def low_from_prob_skill(decoded) -> tuple:
        """(q class 1, q class 2) from best_csi_threshold: decoded is ProbabilitySkill.decode's dict, or a mapping with the `scalars`,
        `scalar_names` and `bins` arrays of a prob_skill.h5.  low[c] = decision_q_from_bin(round(best_csi_threshold_c * bins), bins);
        raises where a class has no threshold (None or NaN)."""
        if "scalars" in decoded:
            names = bytes(np.asarray(decoded["scalar_names"], np.uint8)).decode().split(",")
            col = names.index("best_csi_threshold")
            bins = int(np.asarray(decoded["bins"]).reshape(-1)[0])
            best = [float(np.asarray(decoded["scalars"])[c, col]) for c in (1, 2)]
        else:
            bins = int(decoded["bins"])
            best = [decoded[f"class_{c}"]["best_csi_threshold"] for c in (1, 2)]
        out = []
        for c, t in zip((1, 2), best):
            if t is None or math.isnan(t):
                raise L.DeepcamHipError(f"DecisionRule.from_prob_skill: class {c} has no best_csi_threshold (no pixel scored)")
            out.append(decision_q_from_bin(int(round(t * bins)), bins))
        return tuple(out)

    @classmethod
    def from_prob_skill(cls, decoded, batch: int, height: int, width: int, high=None, connectivity: int = 8, wrap: bool = True,
                        device=None) -> "DecisionRule":
        """The rule whose low thresholds are the best-CSI thresholds of a ProbabilitySkill result (low_from_prob_skill), typically of a
        validation split; as integers q they reproduce the scored forecasts bit for bit."""
        return cls(batch, height, width, low=cls.low_from_prob_skill(decoded), high=high, connectivity=connectivity, wrap=wrap, device=device)

    def thresholds(self) -> dict:
        """q and probability (q / 65536) per class (1, 2)"""
        return {"low_q": list(self.low), "high_q": list(self.high), "low": [q / PROB_ONE for q in self.low],
                "high": [q / PROB_ONE for q in self.high]}

    def __call__(self, logits: torch.Tensor, n_valid: Optional[int] = None) -> torch.Tensor:
        """logits: contiguous device fp32 [B, 3, H, W] (Predictor.logits_buffer).  Returns the uint8 mask [n_valid, H, W], a view of a buffer
        this object owns (mask_buffer is the whole of it; the next call overwrites it).  Samples from n_valid on are neither read nor
        written."""
        check_tensor("DecisionRule", "logits", logits, (torch.float32,), (self.B, 3, self.H, self.W), self.device)
        nv = _n_valid("DecisionRule", n_valid, self.B)
        st = L.stream_ptr()
        L.call("dc_logits_decide", self.B, nv, self.H, self.W, L.dptr(logits), self.low[0], self.low[1], self.high[0], self.high[1],
               L.dptr(self._cand), L.dptr(self._seed) if self.hysteresis else None, L.dptr(self._counts), st)
        self._last_valid = nv
        if nv and self.hysteresis:
            L.call("dc_mask_components", self.B, nv, self.H, self.W, L.dptr(self._cand), self.connectivity, int(self.wrap),
                   L.dptr(self._labels), L.dptr(self._ws), st)
            L.call("dc_hysteresis_select", self.B, nv, self.H, self.W, L.dptr(self._cand), L.dptr(self._seed), L.dptr(self._labels),
                   L.dptr(self._flags), L.dptr(self._out), L.dptr(self._counts), st)
        elif nv:                                  # plain thresholding: every candidate pixel is kept; no events are counted
            c = self._counts[:nv]
            c[:, 2], c[:, 7] = c[:, 0], c[:, 5]
        return self.mask_buffer[:nv]

    @property
    def mask_buffer(self) -> torch.Tensor:
        """uint8 [B, H, W]: the whole buffer the masks are written to, padding samples included (plain thresholding: the candidates')"""
        return self._out if self.hysteresis else self._cand

    @property
    def candidate_buffer(self) -> torch.Tensor:
        """uint8 [B, H, W]: the candidate classes, padding samples included"""
        return self._cand

    def counts(self) -> torch.Tensor:
        """int64 [n_valid, 12] of the last call (a device view, not synchronised): DECISION_COUNTS"""
        return self._counts[:self._last_valid]


# ---------------------------------------------------------------------------------------------- view ensemble
ENSEMBLE_MAX_MEMBERS = 63                         # a 6-bit vote field of the packed state plane
ENSEMBLE_MAX_WEIGHT_SUM = 65535                   # S_c <= sum of weights * 65537 stays below 2^32
ENSEMBLE_ROW = 208                                # 3 x 64 vote cells, then the 4 x 4 (first, pooled) cells
ENSEMBLE_CHANGED = 192


def seam_weights(width: int, roll: int, margin: int) -> np.ndarray:
    """The column weights of a member whose view is rolled by `roll`, uint16 [width] in SOURCE coordinates: min(d + 1, margin), d the
    distance of the pixel's VIEW column to the nearer edge of the view, where the convolutions pad with zeros.  margin = 1 gives all
    ones, the plain mean; a larger margin fades every member out towards its own seam, so that near longitude 0 the rolled views decide."""
    width, roll, margin = int(width), int(roll), int(margin)
    if width < 1 or not 0 <= roll < width or not 1 <= margin <= ENSEMBLE_MAX_WEIGHT_SUM:
        raise L.DeepcamHipError(f"seam_weights: width must be positive, roll in [0, width) and margin in [1, {ENSEMBLE_MAX_WEIGHT_SUM}], "
                                f"got width = {width}, roll = {roll}, margin = {margin}")
    view = (np.arange(width, dtype=np.int64) - roll) % width
    return np.minimum(np.minimum(view, width - 1 - view) + 1, margin).astype(np.uint16)


def view_input(raw: torch.Tensor, channels, shift: torch.Tensor, scale: torch.Tensor, roll: int = 0, flip: bool = False, negate=None,
               out: Optional[torch.Tensor] = None, dtype=None) -> torch.Tensor:
    """One view of the input on the device (dc_input_view_hwc): out[n, h, w, j] = scale[j] * (sign[j] * raw[n, src(h, w), channels[j]] -
    shift[j]) with src(h, w) = (H - 1 - h if flip else h, (w + roll) mod W) -- the input pipeline's normalisation on the rolled and
    mirrored fields.  raw, channels, shift, scale: data.InputPipeline's .raw (fp32 [B, H, W, Cfile]), .channels (device int32 [C], or None:
    the first C file channels), .shift and .scale (device fp32 [C]).  negate: None, the FILE channels whose sign is reversed (a mirrored
    hemisphere reverses the meridional winds), or a device fp32 [C] of +1 / -1.  out: the NHWC tensor [B, H, W, C] of `dtype` that takes
    the view (made when None; dtype defaults to out's, else fp32).  Launches on the current stream and does not synchronise."""
    if not isinstance(raw, torch.Tensor) or raw.dtype != torch.float32 or raw.dim() != 4 or not raw.is_cuda or not raw.is_contiguous():
        raise L.DeepcamHipError("view_input: raw must be a contiguous device fp32 tensor [B, H, W, Cfile]")
    B, H, W, cfile = raw.shape
    C_ = int(shift.numel())
    if dtype is None:
        dtype = out.dtype if out is not None else torch.float32
    if out is None:
        out = torch.empty((B, H, W, C_), dtype=dtype, device=raw.device)
    if tuple(out.shape) != (B, H, W, C_) or out.dtype != dtype or out.device != raw.device or not out.is_contiguous():
        raise L.DeepcamHipError(f"view_input: out must be a contiguous {dtype} tensor {[B, H, W, C_]} on {raw.device}")
    for t, name in ((shift, "shift"), (scale, "scale")):
        if t.dtype != torch.float32 or t.numel() != C_ or t.device != raw.device or not t.is_contiguous():
            raise L.DeepcamHipError(f"view_input: {name} must be a contiguous device fp32 tensor [{C_}]")
    if channels is not None and (channels.dtype != torch.int32 or channels.numel() != C_ or channels.device != raw.device):
        raise L.DeepcamHipError(f"view_input: channels must be None or a device int32 tensor [{C_}]")
    sign = negate
    if negate is not None and not isinstance(negate, torch.Tensor):
        file_channels = list(range(C_)) if channels is None else [int(c) for c in channels.cpu().tolist()]
        wanted = {int(c) for c in negate}
        sign = torch.tensor([-1.0 if c in wanted else 1.0 for c in file_channels], dtype=torch.float32, device=raw.device) if wanted else None
    if sign is not None and (sign.dtype != torch.float32 or sign.numel() != C_ or sign.device != raw.device or not sign.is_contiguous()):
        raise L.DeepcamHipError(f"view_input: negate as a tensor must be a contiguous device fp32 tensor [{C_}] of +1 / -1")
    L.call("dc_input_view_hwc", L.dtype_code(dtype), B, H, W, cfile, C_, L.dptr(channels), L.dptr(sign), L.dptr(raw), L.dptr(shift),
           L.dptr(scale), int(roll), int(bool(flip)), L.dptr(out), C_, L.stream_ptr())
    return out


class ViewEnsemble:
    """Seam-free, test-time-augmented prediction on the device (dc_ensemble_add, dc_ensemble_pool; csrc/ensemble.hip): the classifier's
    fp32 logits of several VIEWS of one batch -- the frame rolled by `roll` columns, an exact symmetry of the periodic grid that only the
    convolutions' zero padding breaks, and mirrored north-south (view_input makes them) -- pooled per pixel of the source frame.  Every
    member adds, per pixel, wt * q_c to three sums S_c (q_c = rint(softmax_c * 65536), ProbabilitySkill's and DecisionRule's integer; wt a
    weight per source column, seam_weights) and one vote for its first-max class; pool() turns the sums into ONE fp32 logits tensor, L_c =
    log(max(S_c, 1) / S_top): its first maximum is the class with the largest S, its softmax is S / sum S to within 0.75 / 65536, and
    predict_from_logits, ProbabilitySkill and DecisionRule take it as they take the classifier's.  A pixel at which a member's logits
    were not finite pools to NaN.  At most 63 members with a sum of their largest weights of at most 65535.  pool() also counts, per frame
    and as running totals since reset(), the pixels with exactly k votes for class c and the (member 0's class, pooled class) matrix.
    Memory: (16 + 12) * batch * height * width bytes.  Nothing here synchronises but a device tensor of weights (its extremes are read)."""

    def __init__(self, batch: int, height: int, width: int, device=None):
        if batch < 1 or batch > PROB_MAX_BATCH or height < 1 or width < 1 or height * width > PROB_MAX_PIXELS:
            raise L.DeepcamHipError(f"ViewEnsemble: batch must lie in [1, {PROB_MAX_BATCH}], height and width be positive and height * width at most 2^30")
        self.B, self.H, self.W = batch, height, width
        dev = torch.device(device_of(device))
        self._state = torch.zeros((batch, 4, height, width), dtype=torch.int32, device=dev)       # uint32 words
        self.device = self._state.device
        self._logits = torch.zeros((batch, 3, height, width), dtype=torch.float32, device=self.device)
        self._rows = torch.zeros((batch, ENSEMBLE_ROW), dtype=torch.int64, device=self.device)
        self._totals = torch.zeros((ENSEMBLE_ROW,), dtype=torch.int64, device=self.device)
        self._frames = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self._weights = {}                            # host arrays already uploaded: bytes -> (device tensor, largest weight)
        self.begin()
        self._pooled_members = self._pooled_valid = 0

    def begin(self) -> "ViewEnsemble":
        """the next add() is member 0 of a new batch"""
        self._members, self._weight_sum, self._nv = 0, 0, None
        return self

    @property
    def members(self) -> int:
        """the members added since begin()"""
        return self._members

    @property
    def state_buffer(self) -> torch.Tensor:
        """int32 [B, 4, H, W] holding the uint32 words of the state: S_0, S_1, S_2 and the packed plane (votes of class 0, 1, 2 in bits
        0-5, 6-11, 12-17, not-finite members in bits 18-23, member 0's class in bits 24-25)"""
        return self._state

    @property
    def logits_buffer(self) -> torch.Tensor:
        """fp32 [B, 3, H, W]: the whole buffer pool() writes, padding samples included"""
        return self._logits

    def _column_weights(self, weights):
        """(device uint16 [W] or None, the largest weight)"""
        if weights is None:
            return None, 1
        if isinstance(weights, torch.Tensor):
            if weights.dtype not in (torch.uint16, torch.int16) or tuple(weights.shape) != (self.W,) or not weights.is_contiguous():
                raise L.DeepcamHipError(f"ViewEnsemble: weights must be a contiguous uint16 tensor [{self.W}]")
            if weights.device == self.device:
                wide = weights.view(torch.int16).to(torch.int32) & 0xFFFF
                lo, hi, dev = int(wide.min()), int(wide.max()), weights
            else:
                return self._column_weights(weights.cpu().view(torch.int16).numpy().view(np.uint16))
        else:
            host = np.ascontiguousarray(weights)
            if host.dtype != np.uint16 or host.shape != (self.W,):
                raise L.DeepcamHipError(f"ViewEnsemble: weights must be uint16 [{self.W}], got {host.dtype} {host.shape}")
            key = host.tobytes()
            if key not in self._weights:
                self._weights[key] = (torch.from_numpy(host.view(np.int16).copy()).to(self.device), int(host.min()), int(host.max()))
            dev, lo, hi = self._weights[key]
        if lo < 1:
            raise L.DeepcamHipError("ViewEnsemble: every weight must be at least 1")
        return dev, hi

    def add(self, logits: torch.Tensor, roll: int = 0, flip: bool = False, weights=None, n_valid: Optional[int] = None) -> "ViewEnsemble":
        """One member: logits, contiguous device fp32 [B, 3, H, W] in the coordinates of the view (roll, flip) they were predicted on;
        weights None (1) or a device or host uint16 [W] per SOURCE column, at least 1.  The first add() after begin() or after
        construction is member 0 and overwrites the state; n_valid must be the same for every member of a batch."""
        shape = (self.B, 3, self.H, self.W)
        if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or tuple(logits.shape) != shape \
                or logits.device != self.device or not logits.is_contiguous():
            got = f"{logits.dtype} {tuple(logits.shape)} on {logits.device}" if isinstance(logits, torch.Tensor) else type(logits).__name__
            raise L.DeepcamHipError(f"ViewEnsemble: logits must be a contiguous torch.float32 tensor {list(shape)} on {self.device}, got {got}")
        nv = _n_valid("ViewEnsemble", n_valid, self.B)
        if self._nv is not None and nv != self._nv:
            raise L.DeepcamHipError(f"ViewEnsemble: member 0 of this batch had n_valid = {self._nv}, got {nv}")
        roll = int(roll)
        if not 0 <= roll < self.W:
            raise L.DeepcamHipError(f"ViewEnsemble: roll must lie in [0, {self.W}), got {roll}")
        dev_weights, largest = self._column_weights(weights)
        if self._members >= ENSEMBLE_MAX_MEMBERS:
            raise L.DeepcamHipError(f"ViewEnsemble: at most {ENSEMBLE_MAX_MEMBERS} members (a vote is a 6-bit field)")
        if self._weight_sum + largest > ENSEMBLE_MAX_WEIGHT_SUM:
            raise L.DeepcamHipError(f"ViewEnsemble: the members' largest weights may sum to at most {ENSEMBLE_MAX_WEIGHT_SUM} (S < 2^32), "
                                    f"got {self._weight_sum} + {largest}")
        L.call("dc_ensemble_add", self.B, nv, self.H, self.W, L.dptr(logits), roll, int(bool(flip)), L.dptr(dev_weights), self._members,
               L.dptr(self._state), L.stream_ptr())
        self._members, self._weight_sum, self._nv = self._members + 1, self._weight_sum + largest, nv
        return self

    def pool(self, n_valid: Optional[int] = None) -> torch.Tensor:
        """The pooled fp32 logits [B, 3, H, W] of the members added since begin(): the whole buffer (logits_buffer; samples from n_valid
        on are not written), overwritten by the next pool().  Adds the frames' counters to the running totals."""
        if self._members < 1:
            raise L.DeepcamHipError("ViewEnsemble: pool() needs at least one member")
        nv = self._nv if n_valid is None else _n_valid("ViewEnsemble", n_valid, self.B)
        if nv != self._nv:
            raise L.DeepcamHipError(f"ViewEnsemble: the members of this batch had n_valid = {self._nv}, got {nv}")
        L.call("dc_ensemble_pool", self.B, nv, self.H, self.W, self._members, L.dptr(self._state), L.dptr(self._logits), L.dptr(self._rows),
               L.dptr(self._totals), L.dptr(self._frames), L.stream_ptr())
        self._pooled_members, self._pooled_valid = self._members, nv
        return self._logits

    def frame_rows(self) -> torch.Tensor:
        """int64 [n_valid, 208] of the last pool(): per frame, word 64 c + k the pixels with exactly k votes for class c, word 192 + 4 i + j
        the pixels whose class in member 0 is i and in the pool j (3: not finite); a view of the object's device buffer, not synchronised"""
        return self._rows[:self._pooled_valid]

    def reset(self) -> None:
        """zeroes the running totals (in stream order)"""
        self._totals.zero_()
        self._frames.zero_()

    def state(self) -> dict:
        """on the host: totals [208] and frames as Python ints, members of the last pool()"""
        return {"totals": [int(v) for v in self._totals.cpu().tolist()], "frames": int(self._frames.cpu()[0]), "members": self._pooled_members}

    def result(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(s["totals"], s["frames"], s["members"])

    @staticmethod
    def decode(totals, frames: int, members: int) -> dict:
        """From the 208 integers: frames, members, pixels, not_finite (pixels at which a member's logits were not finite: they pool to
        NaN); per class ("class_0", "class_1", "class_2") vote_share (a list over k = 0 .. members: the share of pixels with exactly k
        votes for the class), mean_votes, gained (pixels the class has in the pooled mask and not in member 0's) and lost (the reverse);
        unanimous, the share of pixels on which all members name one class; changed, the 4 x 4 matrix [member 0's class][pooled class]
        with 3 = not finite.  A share is None without pixels."""
        t = [int(v) for v in np.asarray(totals).reshape(-1).tolist()]
        members = int(members)
        if len(t) != ENSEMBLE_ROW or not 0 <= members <= ENSEMBLE_MAX_MEMBERS:
            raise L.DeepcamHipError(f"ViewEnsemble.decode: totals must hold {ENSEMBLE_ROW} integers and members lie in [0, {ENSEMBLE_MAX_MEMBERS}]")
        pixels = sum(t[:64])                          # every pixel has some number of votes for class 0
        changed = [[t[ENSEMBLE_CHANGED + 4 * i + j] for j in range(4)] for i in range(4)]
        out = {"frames": int(frames), "members": members, "pixels": pixels, "not_finite": sum(row[3] for row in changed),
               "unanimous": _ratio(sum(t[64 * c + members] for c in range(3)), pixels) if members else None, "changed": changed}
        for c in range(3):
            votes = t[64 * c:64 * c + 64]
            out[f"class_{c}"] = {"vote_share": [_ratio(votes[k], pixels) for k in range(members + 1)],
                                 "mean_votes": _ratio(sum(k * n for k, n in enumerate(votes)), pixels),
                                 "gained": sum(changed[i][c] for i in range(4) if i != c),
                                 "lost": sum(changed[c][j] for j in range(4) if j != c)}
        return out

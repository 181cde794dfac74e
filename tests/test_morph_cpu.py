"""The checker of tests/util_morph.py on hand-made planes, and the host side of nn.MaskMorphology that needs no GPU: the program word,
the C call's refusals, the binding."""
import os

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_morph as um

MM = dnn.MaskMorphology


def _plane(text):
    return np.array([[ch == "#" for ch in row] for row in text.split()])


@pytest.mark.parametrize("wrap", [0, 1])
def test_checker_on_hand_made_planes(wrap):
    ring = _plane("....... .#####. .#...#. .#...#. .#####. .......")
    assert np.array_equal(um.fill(ring, wrap), _plane("....... .#####. .#####. .#####. .#####. ......."))
    cut = ring.copy()
    cut[1, 3] = False                                   # open towards row 0: the inside reaches the pole
    assert np.array_equal(um.fill(cut, wrap), cut)
    for r in (1, 2, 3):                                 # two strips on one row band: a gap of 2r closes, one of 2r + 2 does not
        for gap, joined in ((2 * r, True), (2 * r + 2, False)):
            x = np.zeros((4 * r + 3, 40), bool)
            x[r + 1:3 * r + 2, 4:12] = x[r + 1:3 * r + 2, 12 + gap:30] = True
            closed = um.run_plane(x, MM.closing(r), wrap)
            assert closed[2 * r + 1, 12:12 + gap].all() == joined and (closed >= x).all(), (r, gap)
    x = np.zeros((16, 30), bool)
    x[2:11, 3:12] = True                                # a 9 x 9 blob with a one-pixel tail, and a 2-wide bar
    x[6, 12:16] = x[12:14, 18:27] = True
    kept = um.run_plane(x, MM.opening_by_reconstruction(2), wrap)
    assert np.array_equal(kept[:, :17], x[:, :17]) and not kept[:, 17:].any()
    assert not um.run_plane(x, MM.opening(2), wrap)[6, 12:16].any()      # the plain opening takes the tail
    m = um.noise_mask(24, 70, 2, seed=3)
    for k in (1, 2):
        for b in range(2):
            assert (um.run_plane(m[b] == k, MM.closing(2), wrap) >= (m[b] == k)).all()
            assert (um.run_plane(m[b] == k, MM.opening(2), wrap) <= (m[b] == k)).all()
    out, counts, ran = um.morph(np.array([[[1, 0, 2, 3, 255, 0]]]), [("dilate", 1)], [("dilate", 1)], wrap)
    assert out.tolist() == [[[1, 1, 2, 3, 255, 1 if wrap else 0]]] and not ran.any()    # the pixel both planes claim goes to class 1
    assert counts.tolist() == [[[1, 3 if wrap else 2, 2 if wrap else 1, 0], [1, 1, 0, 0]]]


def test_program_word_round_trip_and_refusals():
    steps = MM.closing(2) + [("fill",)] + MM.opening_by_reconstruction(31)
    word = dnn.morph_program(steps)
    assert word == 0x22 | 0x42 << 8 | 0x60 << 16 | 0x5F << 24 | 0x80 << 32 and dnn.morph_steps(word) == steps
    assert dnn.morph_program([]) == 0 and dnn.morph_program(MM.opening(3)) == 0x2343
    for bad, what in (([("dilate", 0)], "radius"), ([("erode", 32)], "radius"), ([("fill", 1)], "r = 0"), ([(5, 0)], "op 5"),
                      ([("smooth", 1)], "not one of"), ([("fill",)] * 9, "at most 8")):
        with pytest.raises(L.DeepcamHipError, match=what):
            dnn.morph_program(bad)


def test_c_call_refusals_and_binding():
    fn, fake = L.load().dc_mask_morph, 4096
    call = lambda p1=0, p2=0, H=8, W=64, mb=1, wrap=1, out=1 << 30: fn(1, 1, H, W, fake, mb, wrap, p1, p2, out, fake, fake, fake, fake, None)  # noqa: E731
    for kw, what in ((dict(p1=0x4100), "after the end byte"), (dict(p2=0x20), "radius must lie in [1, 31], got 0"), (dict(p1=0xA0), "op 5"),
                     (dict(p2=0xE0 << 56 | 0x41414141414141), "step 7: op 7"), (dict(p1=0x61), "FILL and RECONSTRUCT take r = 0, got 1"), (dict(p1=0x05), "end byte"),
                     (dict(mb=2), "mask_bytes"), (dict(wrap=2), "wrap"), (dict(H=1024, W=2048), "does not fit the LDS"),
                     (dict(out=fake + 8), "alias")):
        assert call(**kw) != 0 and what in L.last_error(), (kw, L.last_error())
    with pytest.raises(L.DeepcamHipError, match=r"op 5 is not defined \(1 DILATE, 2 ERODE, 3 FILL, 4 RECONSTRUCT\)"):
        dnn.morph_program([(5, 0)])                      # the wording of the C call
    assert "dc_mask_morph" in L.EXPORTS and dnn.MORPH_COUNTS == ("pixels_in", "pixels_out", "added", "removed")
    src = os.path.join(L.CSRC, "program_thunks.inc")
    assert '{"dc_mask_morph", &t_dc_mask_morph, 15, "iiiipiillpppppp"}' in open(src).read()

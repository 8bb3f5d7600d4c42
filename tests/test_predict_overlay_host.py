"""CPU: the host side of predict's source-frame outputs - ``heat_lut`` against its documented integer formulas, ``overlay_scale``,
the new flags' parsing (``--save-overlays`` implies ``--source-frame``; the overlay's options go with it), and the numpy overlay
oracle of the GPU tests on a case worked out by hand."""
import numpy as np
import pytest


def test_heat_lut_follows_its_integer_formulas():
    from srad_amd import predict as P
    for alpha_max in (0, 1, 128, 153, 255):
        lut = P.heat_lut(alpha_max)
        assert lut.dtype == np.uint8 and lut.shape == (256, 4)
        alpha = lut[:, 3].astype(int)
        assert alpha[0] == 0 and alpha[255] == alpha_max and (np.diff(alpha) >= 0).all()
        for level in range(256):                              # the docstring, level by level
            seg, t = level // 64, 4 * (level % 64)
            rgb = [(0, t, 255), (0, 255, 255 - t), (t, 255, 0), (255, 255 - t, 0)][seg]
            assert tuple(int(v) for v in lut[level]) == rgb + ((alpha_max * level + 127) // 255,), level
    lut = P.heat_lut(255)
    assert tuple(lut[0]) == (0, 0, 255, 0) and tuple(lut[64]) == (0, 255, 255, 64) and tuple(lut[128]) == (0, 255, 0, 128)
    assert tuple(lut[192]) == (255, 255, 0, 192) and tuple(lut[255]) == (255, 3, 0, 255)
    assert (np.abs(np.diff(lut[:, :3].astype(int), axis=0)).max(axis=1) <= 4).all()       # piecewise linear: no jump in any channel
    for bad in (-1, 256, 0.5, float("nan")):
        with pytest.raises(ValueError, match="alpha_max"):
            P.heat_lut(bad)


def test_overlay_scale():
    from srad_amd import predict as P
    for t in (0.5, 0.1234567, 1.0, 1e-3, float(np.float32(0.3))):
        s = P.overlay_scale(t)
        assert isinstance(s, np.float32) and s == np.float32(127.5 / t)
        assert int(np.float32(t) * s) in (127, 128)           # the threshold sits at the middle of the ramp
    for t in (0.0, -0.25, float("inf"), float("-inf"), float("nan")):
        s = P.overlay_scale(t)
        assert isinstance(s, np.float32) and s == np.float32(255.0), t
    assert np.isfinite(P.overlay_scale(1e-300))


def test_flag_parsing():
    from srad_amd import predict as P
    a = P.parse_predict_args(["--input", "x"])
    assert (a.source_frame, a.save_overlays) == (False, False)
    assert (a.overlay_alpha, a.overlay_contour) == (P.OVERLAY_ALPHA_DEFAULT, P.OVERLAY_CONTOUR_DEFAULT) == (0.6, 1)
    a = P.parse_predict_args(["--input", "x", "--source-frame"])
    assert (a.source_frame, a.save_overlays) == (True, False)
    a = P.parse_predict_args(["--input", "x", "--save-overlays"])
    assert (a.source_frame, a.save_overlays) == (True, True)                        # an overlay is drawn in the source frame
    a = P.parse_predict_args(["--input", "x", "--save-overlays", "--overlay-alpha", "0.25", "--overlay-contour", "0"])
    assert (a.source_frame, a.save_overlays, a.overlay_alpha, a.overlay_contour) == (True, True, 0.25, 0)
    a = P.parse_predict_args(["--input", "x", "--save-overlays", "--overlay-alpha", "1", "--overlay-contour", "4"])
    assert (a.overlay_alpha, a.overlay_contour) == (1.0, 4)
    for bad in (["--input", "x", "--overlay-alpha", "0.5"], ["--input", "x", "--source-frame", "--overlay-contour", "2"],
                ["--input", "x", "--save-overlays", "--overlay-alpha", "1.5"], ["--input", "x", "--save-overlays", "--overlay-alpha", "nan"],
                ["--input", "x", "--save-overlays", "--overlay-alpha", "-0.1"], ["--input", "x", "--save-overlays", "--overlay-contour", "5"],
                ["--input", "x", "--save-overlays", "--overlay-contour", "-1"], ["--input", "x", "--save-overlays", "--overlay-contour", "1.5"]):
        with pytest.raises(SystemExit):
            P.parse_predict_args(bad)


def test_detector_checks_the_overlay_options_before_the_model():
    from srad_amd import predict as P

    class Opt:
        patch_size, scale, n_colors, rgb_range = 32, [2, 4], 1, 255
    with pytest.raises(ValueError, match="alpha_max"):
        P.Detector(Opt(), None, P.MapSpec(ws=7), overlay_alpha=300)
    with pytest.raises(ValueError, match="overlay_contour"):
        P.Detector(Opt(), None, P.MapSpec(ws=7), overlay_contour=5)


def test_overlay_oracle_on_a_case_worked_by_hand():
    from tests.overlay_ref import overlay_ref
    lut = np.zeros((256, 4), dtype=np.uint8)
    lut[0] = 9, 9, 9, 0                                       # alpha 0: the source as it is
    lut[100] = 200, 100, 0, 51                                # (v * 204 + t * 51 + 127) // 255
    lut[255] = 255, 0, 0, 255                                 # alpha 255: the table's colour
    src = np.full((1, 3, 4, 1), 50, dtype=np.uint8)
    maps = np.array([[[0.0, -1.0, np.nan, 100.9], [100.0, 255.0, 1e9, np.inf], [0.5, 99.99, 254.99, 0.0]]], dtype=np.float32)
    masks = np.zeros((1, 3, 4), dtype=np.uint8)
    out = overlay_ref(src, maps, masks, lut, 1.0, 2, (1, 2, 3))
    blend = ((50 * 204 + 200 * 51 + 127) // 255, (50 * 204 + 100 * 51 + 127) // 255, (50 * 204 + 127) // 255)
    assert out[0, 0].tolist() == [[50, 50, 50]] * 3 + [list(blend)]
    assert out[0, 1].tolist() == [list(blend)] + [[255, 0, 0]] * 3
    assert out[0, 2].tolist() == [[50, 50, 50]] * 4                                 # levels 0, 99, 254, 0 have alpha 0 here
    masks[0, :, :] = 1                                        # all set: only the image's border is "outside"
    out = overlay_ref(src, maps, masks, lut, 1.0, 1, (1, 2, 3))
    inner = np.zeros((3, 4), dtype=bool)
    inner[1, 1:3] = True                                      # the two pixels whose 3 x 3 window stays inside the 3 x 4 image
    assert (out[0][~inner] == (1, 2, 3)).all() and (out[0][inner] == (255, 0, 0)).all()
    src5 = np.full((1, 5, 5, 3), 50, dtype=np.uint8)
    m5 = np.ones((1, 5, 5), dtype=np.uint8)
    out = overlay_ref(src5, np.zeros((1, 5, 5), np.float32), m5, lut, 1.0, 1, (1, 2, 3))
    assert (out[0, 1:4, 1:4] == 50).all() and (out[0, 0] == (1, 2, 3)).all() and (out[0, :, 4] == (1, 2, 3)).all()
    m5[0, 2, 2] = 0                                           # a hole: its eight neighbours become contour, the hole does not
    out = overlay_ref(src5, np.zeros((1, 5, 5), np.float32), m5, lut, 1.0, 1, (1, 2, 3))
    assert (out[0, 2, 2] == 50).all() and (out[0, 1, 1] == (1, 2, 3)).all() and (out[0, 3, 2] == (1, 2, 3)).all()
    out0 = overlay_ref(src5, np.zeros((1, 5, 5), np.float32), m5, lut, 1.0, 0, (1, 2, 3))
    assert (out0 == 50).all()                                 # radius 0 draws no contour

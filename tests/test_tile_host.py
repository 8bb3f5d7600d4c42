"""CPU: the tile plan of tiled inference (DESIGN.md "Tiled inference") against its rule, the numpy restatements of gather and
blend that the GPU tests compare the kernels with (checked here against a literal per-pixel loop), the three parsers' flags
and the operating-point file's new entries.  The restatements are written from the definitions in include/srad.h, not from
the kernels."""
import json

import numpy as np
import pytest

PLAN_CASES = [(37, 16, 4, 8), (16, 16, 0, 8), (5, 8, 3, 4), (2, 8, 2, 8), (40, 8, 7, 1),
              (16, 16, 5, 4), (17, 16, 5, 1), (18, 16, 15, 2), (9, 8, 7, 1), (64, 8, 7, 8), (1, 1, 0, 1), (100, 32, 8, 8)]


# ---------------------------------------------------------------- the definitions, restated
def axis_rule(n, T, O, g):
    """(p, t, S, origins) of one axis, as the issue states them."""
    p = -(-n // g) * g
    t = min(T, p)
    S = T - O
    return p, t, S, list(range(0, p - t, S)) + [p - t]


def reflect(i, n):
    j = i % (2 * n)
    return j if j < n else 2 * n - 1 - j


def gather_ref(x, T, O, g):
    """x numpy [B,C,h,w] -> tiles [B*ny*nx, C, ty, tx]: pad by r(), cut at the origins, row-major, image-major."""
    B, C, h, w = x.shape
    py, ty, _, oy = axis_rule(h, T, O, g)
    px, tx, _, ox = axis_rule(w, T, O, g)
    padded = x[:, :, [reflect(i, h) for i in range(py)]][:, :, :, [reflect(i, w) for i in range(px)]]
    return np.stack([padded[b, :, y0:y0 + ty, x0:x0 + tx] for b in range(B) for y0 in oy for x0 in ox])


def axis_weight(E, cap):
    U = np.arange(E, dtype=np.int64)
    return np.minimum(np.minimum(U + 1, E - U), cap)


def blend_ref(y, B, h, w, T, O, g, s, mode):
    """y numpy float32 [B*ny*nx, C, ty*s, tx*s] -> [B,C,h*s,w*s]: the tiles accumulated in tile order, every product and sum
    a float32 operation of numpy, the division float32 / float32; a pixel of one tile is that tile's value."""
    py, ty, _, oy = axis_rule(h, T, O, g)
    px, tx, _, ox = axis_rule(w, T, O, g)
    C, Ey, Ex = y.shape[1], ty * s, tx * s
    assert y.dtype == np.float32 and y.shape == (B * len(oy) * len(ox), C, Ey, Ex)
    wgt = np.outer(axis_weight(Ey, O * s + 1), axis_weight(Ex, O * s + 1)) if mode == "feather" else np.ones((Ey, Ex), np.int64)
    wf = wgt.astype(np.float32)
    assert (wf.astype(np.int64) == wgt).all()                  # every weight an exact fp32 integer
    acc = np.zeros((B, C, py * s, px * s), np.float32)
    first = np.zeros_like(acc)
    count = np.zeros((py * s, px * s), np.int64)
    wsum = np.zeros((py * s, px * s), np.int64)
    k = 0
    for b in range(B):
        count[:], wsum[:] = 0, 0
        for y0 in oy:
            for x0 in ox:
                ys, xs = slice(y0 * s, y0 * s + Ey), slice(x0 * s, x0 * s + Ex)
                term = (wf * y[k]).astype(np.float32) if mode == "feather" else y[k]
                fresh = count[ys, xs] == 0
                acc[b, :, ys, xs] = np.where(fresh, term, (acc[b, :, ys, xs] + term).astype(np.float32))
                first[b, :, ys, xs] = np.where(fresh, y[k], first[b, :, ys, xs])
                count[ys, xs] += 1
                wsum[ys, xs] += wgt
                k += 1
        assert (count >= 1).all()                              # every padded coordinate is covered
        div = (wsum if mode == "feather" else count).astype(np.float32)
        acc[b] = np.where(count == 1, first[b], (acc[b] / div).astype(np.float32))
    return acc[:, :, :h * s, :w * s].copy()


def blend_loop(y, B, h, w, T, O, g, s, mode):
    """The same, literally: one output pixel at a time, its covering tiles visited in tile order."""
    py, ty, _, oy = axis_rule(h, T, O, g)
    px, tx, _, ox = axis_rule(w, T, O, g)
    C, Ey, Ex, cap = y.shape[1], ty * s, tx * s, O * s + 1
    out = np.zeros((B, C, h * s, w * s), np.float32)
    for b in range(B):
        for c in range(C):
            for Y in range(h * s):
                for X in range(w * s):
                    acc, total, n, k = None, 0, 0, b * len(oy) * len(ox)
                    for y0 in oy:
                        for x0 in ox:
                            U, V = Y - y0 * s, X - x0 * s
                            if 0 <= U < Ey and 0 <= V < Ex:
                                v = y[k, c, U, V]
                                wt = min(U + 1, Ey - U, cap) * min(V + 1, Ex - V, cap) if mode == "feather" else 1
                                term = np.float32(wt) * v if mode == "feather" else v
                                acc = term if acc is None else np.float32(acc + term)
                                total, n, only = total + wt, n + 1, v
                            k += 1
                    out[b, c, Y, X] = only if n == 1 else np.float32(acc / np.float32(total))
    return out


# ---------------------------------------------------------------- the plan
@pytest.mark.parametrize("n,T,O,g", PLAN_CASES)
def test_plan_matches_the_rule(n, T, O, g):
    from srad_amd import ops
    p, t, S, origins = axis_rule(n, T, O, g)
    other = (23, 16, 3, 4)                                     # the other axis has its own extent; T, O, g are the call's
    plan = ops.tile_plan(n, 23, T, O, g)
    pw, tw, _, ow = axis_rule(23, T, O, g)
    assert (plan.ph, plan.ty, plan.stride, list(plan.oy), plan.ny) == (p, t, S, origins, len(origins))
    assert (plan.pw, plan.tx, list(plan.ox), plan.nx) == (pw, tw, ow, len(ow))
    flipped = ops.tile_plan(23, n, T, O, g)
    assert (flipped.pw, flipped.tx, list(flipped.ox)) == (p, t, origins) and list(flipped.oy) == ow
    assert len(set(origins)) == len(origins) and origins == sorted(origins)             # no origin twice
    covered = np.zeros(p, bool)
    for o in origins:
        assert 0 <= o and o + t <= p
        covered[o:o + t] = True
    assert covered.all()                                       # every padded coordinate
    assert p % g == 0 and p - n < g and other


def test_reflection_is_numpy_symmetric_where_one_reflection_suffices():
    for n in (1, 2, 3, 5, 8):
        a = np.arange(n)
        for extra in range(0, n + 1):                          # np.pad reflects once up to n extra samples
            want = np.pad(a, (0, extra), mode="symmetric")
            assert [reflect(i, n) for i in range(n + extra)] == want.tolist()
        for i in range(6 * n):                                 # periodic beyond
            assert reflect(i, n) == reflect(i + 2 * n, n) and 0 <= reflect(i, n) < n


def test_refusals_are_value_errors():
    from srad_amd import ops
    for args, what in (((8, 8, 0, 0, 1), "tile must be >= 1"), ((8, 8, -4, 0, 1), "tile must be >= 1"),
                       ((8, 8, 8, 8, 1), "overlap"), ((8, 8, 8, -1, 1), "overlap"), ((8, 8, 12, 2, 8), "granule"),
                       ((8, 8, 8192, 4095, 1, 1), "4094"), ((8, 8, 2048, 1024, 1, 4), "4094")):
        with pytest.raises(ValueError, match=what):
            ops.tile_plan(*args)
    assert ops.tile_plan(8, 8, 8192, 4094, 1, 1).stride == 8192 - 4094
    assert ops.tile_plan(8, 8, 2048, 1023, 1, 4).scale == 4
    with pytest.raises(ValueError, match="mode"):
        ops.tile_blend(None, 8, 8, 8, 0, 1, 1, "median")


# ---------------------------------------------------------------- the restatements against the literal loop
@pytest.mark.parametrize("case", [(2, 2, 5, 7, 4, 2, 2, 2), (1, 1, 3, 2, 4, 1, 4, 1), (1, 2, 6, 6, 3, 2, 1, 3)])
@pytest.mark.parametrize("mode", ["mean", "feather"])
def test_blend_restatement_is_the_pixel_loop(case, mode):
    B, C, h, w, T, O, g, s = case
    x = np.random.RandomState(5).randn(B, C, h, w).astype(np.float32)
    tiles = gather_ref(x, T, O, g)
    py, ty, _, oy = axis_rule(h, T, O, g)
    px, tx, _, ox = axis_rule(w, T, O, g)
    assert tiles.shape == (B * len(oy) * len(ox), C, ty, tx)
    for k, (b, y0, x0) in enumerate((b, y0, x0) for b in range(B) for y0 in oy for x0 in ox):     # gather, literally
        for u in range(ty):
            for v in range(tx):
                assert (tiles[k, :, u, v] == x[b, :, reflect(y0 + u, h), reflect(x0 + v, w)]).all()
    y = np.random.RandomState(6).randn(tiles.shape[0], C, ty * s, tx * s).astype(np.float32)
    got, want = blend_ref(y, B, h, w, T, O, g, s, mode), blend_loop(y, B, h, w, T, O, g, s, mode)
    assert got.dtype == np.float32 and got.shape == (B, C, h * s, w * s)
    assert np.array_equal(got, want)


def test_blend_of_gather_returns_the_image():
    x = np.random.RandomState(7).randint(-64, 65, (2, 1, 11, 13)).astype(np.float32)
    for mode in ("mean", "feather"):
        assert np.array_equal(blend_ref(gather_ref(x, 8, 3, 4), 2, 11, 13, 8, 3, 4, 1, mode), x)


# ---------------------------------------------------------------- flags
def test_the_three_parsers_agree_and_default_to_off():
    from srad_amd import options as O
    from srad_amd import predict as P
    parsers = (lambda a: O.parse_train_args(a), lambda a: O.parse_eval_args(a), lambda a: P.parse_predict_args(["--input", "x"] + a))
    for parse in parsers:
        off = parse([])
        assert (off.tile, off.tile_overlap, off.tile_blend) == (0, 0, "mean")
        on = parse(["--tile", "32", "--tile-overlap", "8", "--tile-blend", "feather"])
        assert (on.tile, on.tile_overlap, on.tile_blend) == (32, 8, "feather")
        assert (parse(["--tile", "32"]).tile_overlap, parse(["--tile", "32"]).tile_blend) == (0, "mean")
        for bad in (["--tile-overlap", "4"], ["--tile-blend", "feather"], ["--tile-blend", "mean"], ["--tile", "0", "--tile-overlap", "0"],
                    ["--tile", "8", "--tile-overlap", "8"], ["--tile", "-8"], ["--tile", "8", "--tile-blend", "median"],
                    ["--tile", "8", "--tile-overlap", "-1"]):
            with pytest.raises(SystemExit):
                parse(bad)
    assert P.parse_predict_args(["--input", "x"]).frame is None
    assert P.parse_predict_args(["--input", "x", "--frame", "48", "80"]).frame == [48, 80]
    with pytest.raises(SystemExit):
        P.parse_predict_args(["--input", "x", "--frame", "48"])
    with pytest.raises(SystemExit):
        P.parse_predict_args(["--input", "x", "--frame", "0", "80"])


def test_config_file_values_get_the_command_lines_checks(tmp_path):
    from srad_amd import options as O
    cfg = tmp_path / "c.yaml"
    cfg.write_text("tile: 16\ntile-overlap: 4\ntile-blend: feather\n")
    for parse in (O.parse_train_args, O.parse_eval_args):
        a = parse(["--config", str(cfg)])
        assert (a.tile, a.tile_overlap, a.tile_blend) == (16, 4, "feather")
    for text in ("tile: 16\ntile-overlap: 16\n", "tile-overlap: 4\n", "tile: 16\ntile-blend: median\n", "tile: -1\n", "tile: x\n"):
        cfg.write_text(text)
        for parse in (O.parse_train_args, O.parse_eval_args):
            with pytest.raises(SystemExit):
                parse(["--config", str(cfg)])


def test_option_object_carries_the_setting_only_when_on():
    from srad_amd import main as Main
    from srad_amd import options as O
    off = Main.build_train_opt(O.parse_train_args([]))
    assert not any(k.startswith("tile") for k in vars(off))    # config.txt lists vars(opt): a run without the flag writes today's file
    on = Main.build_train_opt(O.parse_train_args(["--tile", "32", "--tile-overlap", "8"]))
    assert (on.tile, on.tile_overlap, on.tile_blend) == (32, 8, "mean")

    class M:
        tile, tile_overlap, tile_blend = 32, 8, "feather"
    assert O.tile_suffix(M()) == " (tiles 32/8 feather)"
    M.tile = 0
    assert O.tile_suffix(M()) == "" and O.tile_suffix(object()) == ""


# ---------------------------------------------------------------- operating_point.json
def test_operating_point_file_tile_and_frame_entries(tmp_path):
    from srad_amd import predict as P
    f = tmp_path / P.OPERATING_POINT_FILE
    spec = P.MapSpec(ws=11)
    P.write_operating_point(f, 0.25, 0.01, "pixel", 0.01, 4, 1, spec, False, "m.pt")
    raw = json.loads(f.read_text())
    assert "tile" not in raw and "frame" not in raw            # off: the file as it always was
    old = P.read_operating_point(f)
    assert old["tile"] is None and old["frame"] is None        # files without the keys read as off
    plain = P.parse_predict_args(["--input", "x"])
    assert P.tile_from_args(plain, old) == (None, None) and P.tile_from_args(plain) == (None, None)
    tiled = P.parse_predict_args(["--input", "x", "--tile", "32", "--tile-overlap", "8", "--tile-blend", "feather", "--frame", "48", "80"])
    assert P.tile_from_args(tiled) == ((32, 8, "feather"), (48, 80))
    with pytest.raises(ValueError, match="--tile 32 .* contradicts the calibrated operating point .*without tiling"):
        P.tile_from_args(tiled, old)
    with pytest.raises(ValueError, match="--frame 48 80 contradicts the calibrated operating point"):
        P.tile_from_args(P.parse_predict_args(["--input", "x", "--frame", "48", "80"]), old)

    P.write_operating_point(f, 0.25, 0.01, "pixel", 0.01, 4, 1, spec, False, "m.pt", tile=(32, 8, "feather"), frame=(48, 80))
    raw = json.loads(f.read_text())
    assert raw["tile"] == [32, 8, "feather"] and raw["frame"] == [48, 80]
    new = P.read_operating_point(f)
    assert new["tile"] == (32, 8, "feather") and new["frame"] == (48, 80)
    assert P.tile_from_args(plain, new) == ((32, 8, "feather"), (48, 80))          # the stored setting is taken
    assert P.tile_from_args(tiled, new) == ((32, 8, "feather"), (48, 80))          # the same flags pass
    for flags in (["--tile", "16"], ["--tile", "32", "--tile-overlap", "4", "--tile-blend", "feather"], ["--tile", "32", "--tile-overlap", "8"]):
        with pytest.raises(ValueError, match="--tile .* contradicts the calibrated operating point"):
            P.tile_from_args(P.parse_predict_args(["--input", "x"] + flags), new)
    with pytest.raises(ValueError, match="--frame 80 48 contradicts"):
        P.tile_from_args(P.parse_predict_args(["--input", "x", "--frame", "80", "48"]), new)


def test_detector_frame_is_checked_on_the_host():
    from srad_amd import predict as P

    class Opt:
        patch_size, scale, n_colors, rgb_range = 64, 4, 1, 255

    class Mdl:
        device = "cpu"

        def eval(self):
            return self
    det = P.Detector(Opt(), Mdl(), P.MapSpec(ws=11), hr_size=(50, 81))
    assert det.frame == (50, 81) and det.lr_frame == (12, 20) and det.hr_size == (50, 81)
    assert P.Detector(Opt(), Mdl(), P.MapSpec(ws=11)).hr_size == 64 and P.Detector(Opt(), Mdl(), P.MapSpec(ws=11), hr_size=32).frame == (32, 32)
    with pytest.raises(ValueError, match="below the scale"):
        P.Detector(Opt(), Mdl(), P.MapSpec(ws=11), hr_size=(3, 80))
    with pytest.raises(ValueError, match="map scales"):        # the spec is resolved against the frame
        P.Detector(Opt(), Mdl(), P.MapSpec(scales=[7, 99]), hr_size=(48, 80))
    assert P.Detector(Opt(), Mdl(), P.MapSpec(scales="sweep"), hr_size=(48, 80)).spec.scales == P.MapSpec(scales="sweep").resolve(48, 80).scales

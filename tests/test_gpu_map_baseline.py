"""GPU: the three baseline kernels (srad_map_stats_accumulate, srad_map_normalize, srad_map_normalize_loo; DESIGN.md
"Baseline") through srad_amd.metrics, bit for bit against the numpy restatement of tests/baseline_ref.py: shapes that take the
scalar instance (5 x 7, 33 x 45: H * W is no multiple of 4) and the four-pixel instance (64 x 64, more than one workgroup),
1, 3 and 7 images (the accumulation walks four images at a time), tensors that start 4 bytes off a 16-byte boundary (the
scalar instance at 64 x 64), in place; batch invariance of the sums; NaN; signed maxima; the pixel AUC of signed maps; the
band-and-blob case through MapBaseline; the argument errors."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import baseline_ref as R

pytestmark = pytest.mark.gpu

SHAPES = ((5, 7), (33, 45), (64, 64))
COUNTS = (1, 3, 7)
N_TOTAL, FLOOR_REL = 9, 0.1


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Per shape, computed once: 9 calibration maps (signed, so z and the maxima have both signs), their reference sums and
    planes, and the reference results for the first 7 of them."""
    H, W = shape
    rng = np.random.default_rng(H * 100 + W)
    base = rng.uniform(-0.3, 0.6, (H, W))
    maps = (base[None] + rng.uniform(0.01, 0.2, (H, W))[None] * rng.standard_normal((N_TOTAL, H, W))).astype(np.float32)
    maps[:, 0, 0] = np.float32(0.125)                         # a pixel that never varies: the floor decides its spread
    s1, s2 = R.sums_ref(maps)
    p = R.planes_ref(s1, s2, N_TOTAL, FLOOR_REL)
    return dict(maps=maps, s1=s1, s2=s2, p=p, z=R.apply_ref(maps[:7], p["mu32"], p["inv32"]),
                loo=R.loo_ref(maps[:7], s1, s2, N_TOTAL, p["floor"]))


def _dev(a, off=False):
    """The array on the GPU; ``off``: in a buffer that starts one element late, so 4 (float32) or 8 (float64) bytes off a
    16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        d = t.cuda()
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    d = buf[1:].view(t.shape)
    d.copy_(t)
    assert d.data_ptr() % 16 == t.element_size() and d.is_contiguous()
    return d


@pytest.mark.parametrize("off", [False, True], ids=["aligned", "off4"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_entry_points_bit_for_bit(shape, off):
    from srad_amd import metrics as M
    c = _case(shape)
    mu, inv = _dev(c["p"]["mu32"]), _dev(c["p"]["inv32"])
    s1, s2 = _dev(c["s1"]), _dev(c["s2"])
    for n in COUNTS:
        maps = _dev(c["maps"][:n], off)
        # accumulate: from nothing, and onto given sums
        a1, a2 = M.map_stats_accumulate(maps)
        w1, w2 = R.sums_ref(c["maps"][:n])
        assert a1.dtype == torch.float64 and tuple(a1.shape) == shape
        assert R.same_bits(a1.cpu().numpy(), w1) and R.same_bits(a2.cpu().numpy(), w2), (shape, n, "sums")
        b1, b2 = M.map_stats_accumulate(maps, a1, a2)
        assert b1 is a1 and b2 is a2
        w1, w2 = R.sums_ref(c["maps"][:n], w1, w2)
        assert R.same_bits(a1.cpu().numpy(), w1) and R.same_bits(a2.cpu().numpy(), w2), (shape, n, "sums onto sums")
        # apply
        z, zmax = M.normalize_maps(maps, mu, inv, with_max=True)
        assert R.same_bits(z.cpu().numpy(), c["z"][:n]), (shape, n, "apply")
        assert R.same_max(zmax.cpu().numpy(), R.max_ref(c["z"][:n])), (shape, n, "apply max")
        assert torch.equal(M.normalize_maps(maps, mu, inv), z)
        # leave-one-out
        q, qmax = M.normalize_maps_loo(maps, s1, s2, N_TOTAL, c["p"]["floor"], with_max=True)
        assert R.same_bits(q.cpu().numpy(), c["loo"][:n]), (shape, n, "leave-one-out")
        assert R.same_max(qmax.cpu().numpy(), R.max_ref(c["loo"][:n])), (shape, n, "leave-one-out max")
        assert torch.equal(M.normalize_maps_loo(maps, s1, s2, N_TOTAL, c["p"]["floor"]), q)
        # in place
        back = M.normalize_maps(maps, mu, inv, out=maps)
        assert back.data_ptr() == maps.data_ptr() and torch.equal(maps, z), (shape, n, "in place")
    assert (c["z"] < 0).any() and (c["z"] > 0).any() and (R.max_ref(c["loo"]) > 0).all()
    assert c["p"]["inv32"][0, 0] == np.float32(1.0 / c["p"]["floor"])          # the floored pixel


@pytest.mark.parametrize("shape", [(33, 45), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_misaligned_planes_take_the_scalar_instance_with_the_same_bits(shape):
    from srad_amd import metrics as M
    c = _case(shape)
    maps = _dev(c["maps"][:7])
    z = M.normalize_maps(maps, _dev(c["p"]["mu32"], True), _dev(c["p"]["inv32"], True))
    assert R.same_bits(z.cpu().numpy(), c["z"])
    q = M.normalize_maps_loo(maps, _dev(c["s1"], True), _dev(c["s2"], True), N_TOTAL, c["p"]["floor"])
    assert R.same_bits(q.cpu().numpy(), c["loo"])
    a1, a2 = _dev(np.zeros(shape), True), _dev(np.zeros(shape), True)
    M.map_stats_accumulate(maps, a1, a2)
    w1, w2 = R.sums_ref(c["maps"][:7])
    assert R.same_bits(a1.cpu().numpy(), w1) and R.same_bits(a2.cpu().numpy(), w2)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_accumulate_is_batch_invariant(shape):
    from srad_amd import metrics as M
    maps = _dev(_case(shape)["maps"][:7])
    one = M.map_stats_accumulate(maps)
    split = M.map_stats_accumulate(maps[3:], *M.map_stats_accumulate(maps[:3]))
    single = (None, None)
    for i in range(7):
        single = M.map_stats_accumulate(maps[i:i + 1], *single)
    for a, b, c in zip(one, split, single):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(a.view(torch.int64), c.view(torch.int64))


def test_nan_pixel_stays_in_its_pixel_and_its_image():
    from srad_amd import metrics as M
    c = _case((33, 45))
    maps = c["maps"][:7].copy()
    maps[2, 5, 6] = np.nan
    d = _dev(maps)
    s1, s2 = M.map_stats_accumulate(d)
    for s in (s1, s2):
        nan = torch.isnan(s).cpu().numpy()
        assert nan[5, 6] and nan.sum() == 1
    w1, w2 = R.sums_ref(maps)
    assert R.same_bits(s1.cpu().numpy(), w1) and R.same_bits(s2.cpu().numpy(), w2)
    z, zmax = M.normalize_maps(d, _dev(c["p"]["mu32"]), _dev(c["p"]["inv32"]), with_max=True)
    want = R.apply_ref(maps, c["p"]["mu32"], c["p"]["inv32"])
    assert R.same_bits(z.cpu().numpy(), want) and np.isnan(want).sum() == 1
    assert R.same_max(zmax.cpu().numpy(), R.max_ref(want)) and np.isnan(zmax.cpu().numpy()).tolist() == [k == 2 for k in range(7)]
    q, qmax = M.normalize_maps_loo(d, _dev(c["s1"]), _dev(c["s2"]), N_TOTAL, c["p"]["floor"], with_max=True)
    want = R.loo_ref(maps, c["s1"], c["s2"], N_TOTAL, c["p"]["floor"])
    assert R.same_bits(q.cpu().numpy(), want) and np.isnan(qmax.cpu().numpy()).tolist() == [k == 2 for k in range(7)]
    # NaN sums (a NaN among the calibration maps) give NaN leave-one-out scores at that pixel in every image
    q = M.normalize_maps_loo(_dev(c["maps"][:3]), s1, s2, 7, c["p"]["floor"])
    assert torch.isnan(q[:, 5, 6]).all() and int(torch.isnan(q).sum()) == 3


def test_maxima_of_negative_maps_and_signed_pixel_auc():
    from srad_amd import metrics as M
    c = _case((33, 45))
    low = (c["maps"][:7] - np.float32(3.0)).astype(np.float32)                # every z below zero
    z, zmax = M.normalize_maps(_dev(low), _dev(c["p"]["mu32"]), _dev(c["p"]["inv32"]), with_max=True)
    want = R.apply_ref(low, c["p"]["mu32"], c["p"]["inv32"])
    assert (want < 0).all() and R.same_bits(z.cpu().numpy(), want) and R.same_max(zmax.cpu().numpy(), R.max_ref(want))
    labels = (np.random.default_rng(3).random(c["z"].shape) < 0.2).astype(np.uint8)
    signed = _dev(c["z"])
    assert M.pixel_roc_auc(signed, _dev(labels)) == R.pixel_auc(c["z"], labels)


def test_band_and_blob_through_map_baseline():
    from srad_amd import baseline as B
    from srad_amd import metrics as M
    calib, good, bad, masks = R.band_and_blob(seed=0)
    raw = R.auc(R.max_ref(good), R.max_ref(bad))
    b = B.MapBaseline(0.1).update(_dev(calib[:5])).update(_dev(calib[5:]))     # a fit in chunks
    whole = B.MapBaseline.fit(_dev(calib), 0.1)
    s1, s2 = R.sums_ref(calib)
    p = R.planes_ref(s1, s2, len(calib), 0.1)
    for fitted in (b, whole):
        assert fitted.n == 12 and R.same_bits(fitted.s1.cpu().numpy(), s1) and R.same_bits(fitted.s2.cpu().numpy(), s2)
        assert R.same_bits(fitted.planes()["mu32"], p["mu32"]) and R.same_bits(fitted.planes()["inv32"], p["inv32"])
        assert fitted.entries() == dict(map_baseline=dict(n_images=12, floor_rel=0.1, floor=p["floor"], pooled_sd=p["pooled"]))
    zg, gmax = whole.apply(_dev(good), with_max=True)
    zb, bmax = whole.apply(_dev(bad), with_max=True)
    assert R.same_bits(zb.cpu().numpy(), R.apply_ref(bad, p["mu32"], p["inv32"]))
    norm = R.auc(gmax.cpu().numpy(), bmax.cpu().numpy())
    assert raw <= 0.6 and norm == 1.0, (raw, norm)
    loo, lmax = whole.apply_loo(_dev(calib), with_max=True)
    assert R.same_bits(loo.cpu().numpy(), R.loo_ref(calib, s1, s2, 12, p["floor"]))
    # a pixel threshold from the leave-one-out maps finds every blob; it lies above the in-sample one at the same rate (leaving
    # a map out moves its own z away from zero: |z_loo| >= |z| at every pixel for n >= 3), which Samuelson's bound caps
    t, _ = M.map_threshold(loo, 0.001)
    t_in, _ = M.map_threshold(whole.apply(_dev(calib)), 0.001)
    hit = (zb > t).cpu().numpy().astype(bool)
    assert all(hit[k][masks[k] == 1].all() for k in range(len(bad)))
    assert t_in <= 11 / np.sqrt(12) * (1 + 1e-5) and t > t_in
    with pytest.raises(ValueError, match=r"\(32, 32\)"):
        whole.apply(torch.zeros(2, 16, 16, device="cuda"))
    with pytest.raises(ValueError, match="do not vary"):
        B.MapBaseline.fit(torch.full((3, 8, 8), 0.5, device="cuda"))


def test_argument_errors():
    from srad_amd import _lib as L
    from srad_amd import metrics as M
    lib = L.lib()
    m = torch.rand(3, 8, 8, device="cuda")
    f32, f64 = torch.rand(8, 8, device="cuda"), torch.rand(8, 8, device="cuda", dtype=torch.float64)
    for call in (lambda: M.map_stats_accumulate(m.double()), lambda: M.map_stats_accumulate(m[0]), lambda: M.map_stats_accumulate(m, f64),
                 lambda: M.map_stats_accumulate(m, f32, f32), lambda: M.map_stats_accumulate(m, f64[:4], f64[:4]),
                 lambda: M.normalize_maps(m, f64, f32), lambda: M.normalize_maps(m, f32, f32[:, :4]),
                 lambda: M.normalize_maps(m, f32, f32, out=m[:2]), lambda: M.normalize_maps(m, f32, f32, out=m.double()),
                 lambda: M.normalize_maps_loo(m, f32, f64, 3, 0.1), lambda: M.normalize_maps_loo(m, f64, f64, 2, 0.1),
                 lambda: M.normalize_maps_loo(m, f64, f64, 3, 0.0), lambda: M.normalize_maps_loo(m, f64, f64, 3, float("nan")),
                 lambda: M.normalize_maps_loo(m, f64, f64, 3, float("inf"))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError, match="GPU only"):
        M.normalize_maps(m.cpu(), f32, f32)
    # the C entry points refuse before any launch: nothing below is ever dereferenced
    p, q, r, o = (C.c_void_p(v << 20) for v in (1, 2, 3, 4))
    nb, ws = C.c_size_t(), C.c_size_t(256)
    err = lambda: lib.srad_last_error()
    assert lib.srad_map_normalize_workspace_bytes(3, C.byref(nb)) == 0 and nb.value >= 3 * 4
    assert lib.srad_map_normalize_workspace_bytes(3, None) == 1 and lib.srad_map_normalize_workspace_bytes(0, C.byref(nb)) == 1
    for args in ((None, 1, 8, 8, q, r, None), (p, 1, 8, 8, None, r, None), (p, 1, 8, 8, q, None, None), (p, 0, 8, 8, q, r, None),
                 (p, 1, 0, 8, q, r, None), (p, 1, 8, -1, q, r, None), (p, 1 << 11, 1 << 10, 1 << 10, q, r, None),
                 (p, 1, 8, 8, q, q, None), (p, 1, 8, 8, C.c_void_p((1 << 20) + 64), r, None)):
        assert lib.srad_map_stats_accumulate(*args) == 1 and b"map_stats_accumulate" in err(), args
    for args in ((None, 1, 8, 8, q, r, o, None, p, ws, None), (p, 1, 8, 8, None, r, o, None, p, ws, None), (p, 1, 8, 8, q, None, o, None, p, ws, None),
                 (p, 1, 8, 8, q, r, None, None, p, ws, None), (p, 0, 8, 8, q, r, o, None, p, ws, None), (p, 1, 8, 0, q, r, o, None, p, ws, None),
                 (p, 2, 8, 8, q, r, C.c_void_p((1 << 20) + 8), None, p, ws, None),          # a partial overlap of out and maps
                 (p, 1, 8, 8, q, r, q, None, p, ws, None),                                   # out on a plane
                 (p, 1, 8, 8, q, r, o, r, None, ws, None), (p, 1, 8, 8, q, r, o, r, p, C.c_size_t(0), None)):      # a maximum without a workspace
        assert lib.srad_map_normalize(*args) == 1 and b"map_normalize" in err(), args
    fl = C.c_double(0.5)
    for args in ((None, 1, 8, 8, q, r, 3, fl, o, None, p, ws, None), (p, 1, 8, 8, None, r, 3, fl, o, None, p, ws, None),
                 (p, 1, 8, 8, q, r, 3, fl, None, None, p, ws, None), (p, 1, 8, 8, q, r, 2, fl, o, None, p, ws, None),
                 (p, 1, 8, 8, q, r, 3, C.c_double(0.0), o, None, p, ws, None), (p, 1, 8, 8, q, r, 3, C.c_double(-1.0), o, None, p, ws, None),
                 (p, 1, 8, 8, q, r, 3, C.c_double(float("nan")), o, None, p, ws, None),
                 (p, 1, -8, 8, q, r, 3, fl, o, None, p, ws, None), (p, 1, 8, 8, q, r, 3, fl, r, None, p, ws, None)):
        assert lib.srad_map_normalize_loo(*args) == 1 and b"map_normalize_loo" in err(), args

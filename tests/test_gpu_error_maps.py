"""GPU: squared-error maps (srad_error_maps / srad_error_maps_multi; DESIGN.md "Squared-error maps").  On u8 images the window
sum of the squared error is an integer, so the map is defined bit for bit: every comparison below is ``torch.equal`` with a numpy
restatement (int64 squared error, ``np.pad(..., mode="reflect")`` with the asymmetric pad of an even window, a window sum,
``np.float32(S * inv)``), which ``test_restatement_against_a_double_loop`` first checks on the CPU against a literal loop."""
import numpy as np
import pytest
import torch


def sqerr(sr, hr):
    """e[n, i, j] = sum_c (sr - hr)^2 as int64, from u8 [n, H, W, C] arrays."""
    d = sr.astype(np.int64) - hr.astype(np.int64)
    return (d * d).sum(-1)


def window_sums(e, ws):
    """S[n, i, j] = the sum of e over rows i - ws//2 .. i + ws - 1 - ws//2 and the columns likewise, numpy reflect padding."""
    lo, hi = ws // 2, ws - 1 - ws // 2
    p = np.pad(e, ((0, 0), (lo, hi), (lo, hi)), mode="reflect")
    c = np.zeros((p.shape[0], p.shape[1] + 1, p.shape[2] + 1), dtype=np.int64)
    c[:, 1:, 1:] = p.cumsum(1).cumsum(2)
    H, W = e.shape[1:]
    return c[:, ws:ws + H, ws:ws + W] - c[:, :H, ws:ws + W] - c[:, ws:ws + H, :W] + c[:, :H, :W]


def error_map_ref(sr, hr, ws):
    """The definition: float32(float64(S) * inv) with inv = 1.0 / (C * ws * ws * 65025) in double."""
    inv = 1.0 / (sr.shape[-1] * ws * ws * 65025)
    return np.float32(window_sums(sqerr(sr, hr), ws).astype(np.float64) * inv)


def multi_ref(sr, hr, sizes, reduce):
    acc = error_map_ref(sr, hr, sizes[0])
    for ws in sizes[1:]:
        m = error_map_ref(sr, hr, ws)
        acc = np.maximum(acc, m) if reduce == "max" else acc + m          # float32 + float32 -> float32
    return acc * np.float32(1.0 / len(sizes)) if reduce == "mean" else acc


def random_pairs(n, H, W, C, seed):
    g = np.random.default_rng(seed)
    hr = g.integers(0, 256, (n, H, W, C), dtype=np.uint8)
    sr = g.integers(0, 256, (n, H, W, C), dtype=np.uint8)
    sr[0] = np.clip(hr[0].astype(np.int64) + g.integers(-6, 7, hr[0].shape), 0, 255).astype(np.uint8)    # one near pair
    return sr, hr


def test_restatement_against_a_double_loop():
    """CPU: the restatement the GPU tests rely on equals the literal definition at 9 x 7, odd, even and all-reflecting windows."""
    sr, hr = random_pairs(2, 9, 7, 3, seed=1)
    e = sqerr(sr, hr)
    H, W = 9, 7

    def refl(k, n):
        return -k if k < 0 else 2 * (n - 1) - k if k > n - 1 else k
    for ws in (1, 2, 3, 4, 5, 11, 13):
        lo = ws // 2
        want = np.zeros_like(e)
        for n in range(2):
            for i in range(H):
                for j in range(W):
                    want[n, i, j] = sum(int(e[n, refl(i - lo + a, H), refl(j - lo + b, W)]) for a in range(ws) for b in range(ws))
        assert np.array_equal(window_sums(e, ws), want), ws
        assert np.array_equal(error_map_ref(sr, hr, ws), np.float32(want.astype(np.float64) * (1.0 / (3 * ws * ws * 65025)))), ws


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


SHAPES = [(33, 45, 1), (64, 64, 3), (128, 128, 1)]           # per-lane path (width not a multiple of 64); scalar-row path; gray


def _sizes(H, W):
    return [1, 3, 4, 11, 2 * min(H, W) - 1]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C", SHAPES)
def test_equal_to_the_definition(H, W, C):
    from srad_amd import metrics as M
    sr, hr = random_pairs(3, H, W, C, seed=H + C)
    dsr, dhr = _dev(sr), _dev(hr)
    for ws in _sizes(H, W):
        got = M.error_maps(dsr, dhr, ws)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, H, W)
        assert torch.equal(got.cpu(), torch.from_numpy(error_map_ref(sr, hr, ws))), (H, W, C, ws)
    assert torch.equal(M.error_maps(dsr, dhr), M.error_maps(dsr, dhr, 1))           # ws defaults to the raw squared error
    # stacks that do not start on a 4-byte boundary: the ws 1 launch then reads byte by byte (and 3 images of 33 x 45 are 4455
    # pixels, no multiple of 4: the last group of the aligned launch above was a partial one)
    if C == 1:
        flat_s, flat_h = torch.zeros(sr.size + 1, dtype=torch.uint8).cuda(), torch.zeros(hr.size + 1, dtype=torch.uint8).cuda()
        flat_s[1:], flat_h[1:] = dsr.reshape(-1), dhr.reshape(-1)
        off_s, off_h = flat_s[1:].view(3, H, W, C), flat_h[1:].view(3, H, W, C)
        assert off_s.data_ptr() % 4 == 1 and off_s.is_contiguous()
        for ws in (1, 3):
            assert torch.equal(M.error_maps(off_s, off_h, ws).cpu(), torch.from_numpy(error_map_ref(sr, hr, ws))), ws


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C", SHAPES)
def test_one_differing_pixel(H, W, C):
    """Identical images but for one pixel, away from the edges: the map is zero outside that pixel's windows and fp32(d^2 * inv)
    inside them (the window that spans the image is checked against the restatement only)."""
    from srad_amd import metrics as M
    g = np.random.default_rng(5)
    hr = g.integers(0, 256, (1, H, W, C), dtype=np.uint8)
    sr = hr.copy()
    y, x, d = H // 2 + 1, W // 3, 37
    sr[0, y, x, 0] = np.uint8((int(hr[0, y, x, 0]) + d) % 256)
    d2 = (int(sr[0, y, x, 0]) - int(hr[0, y, x, 0])) ** 2
    for ws in _sizes(H, W):
        got = M.error_maps(_dev(sr), _dev(hr), ws).cpu().numpy()
        assert np.array_equal(got, error_map_ref(sr, hr, ws)), ws
        lo, hi = ws // 2, ws - 1 - ws // 2
        inv = 1.0 / (C * ws * ws * 65025)
        if ws <= 11:                                         # no window that holds (y, x) reaches an edge: it holds it once
            assert ws - 1 <= y <= H - ws and ws - 1 <= x <= W - ws
            inside = np.zeros((H, W), dtype=bool)
            inside[y - hi:y + lo + 1, x - hi:x + lo + 1] = True
            assert np.all(got[0][~inside] == 0.0), ws
            assert np.all(got[0][inside] == np.float32(d2 * inv)), ws


@pytest.mark.gpu
def test_wide_sums():
    """RGB 256 x 256, sr = 0, hr = 255: S = 3 * 65025 * ws^2 passes 2^32 at ws 255 (1.27e10), which a 32-bit table or
    accumulator cannot hold.  Every value is 1 to within one ulp."""
    from srad_amd import metrics as M
    sr, hr = np.zeros((1, 256, 256, 3), np.uint8), np.full((1, 256, 256, 3), 255, np.uint8)
    assert 3 * 65025 * 255 ** 2 > 2 ** 32
    for ws in (255, 511):
        got = M.error_maps(_dev(sr), _dev(hr), ws).cpu().numpy()
        assert np.array_equal(got, error_map_ref(sr, hr, ws)), ws
        assert np.all(np.abs(got.astype(np.float64) - 1.0) <= 2.0 ** -23), ws
    # and with content: random images at the same sizes
    sr, hr = random_pairs(1, 256, 256, 3, seed=9)
    for ws in (255, 511):
        assert np.array_equal(M.error_maps(_dev(sr), _dev(hr), ws).cpu().numpy(), error_map_ref(sr, hr, ws)), ws


TWENTY = list(range(3, 42, 2))                               # 20 sizes: two launches (16 + 4)
SEVENTEEN = [3] * 16 + [11]                                  # a second launch of exactly one size, continued from the stored accumulator


def _compose(sr, hr, sizes, reduce):
    from srad_amd import metrics as M
    acc = M.error_maps(sr, hr, sizes[0])
    for ws in sizes[1:]:
        m = M.error_maps(sr, hr, ws)
        acc = torch.maximum(acc, m) if reduce == "max" else acc + m
    if reduce == "mean":
        acc = acc * torch.tensor(np.float32(1.0 / len(sizes)), device=acc.device)
    return acc


@pytest.mark.gpu
@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("H,W,C", [(64, 64, 3), (33, 45, 1)])
def test_multi_scale_equals_the_composition(H, W, C, reduce):
    from srad_amd import metrics as M
    assert len(TWENTY) == 20
    sr, hr = random_pairs(2, H, W, C, seed=11)
    dsr, dhr = _dev(sr), _dev(hr)
    for sizes in ([11], [3, 11, 21], [21, 3, 11], [5, 5], TWENTY, SEVENTEEN, [1], [1, 4]):
        got = M.error_maps_multi(dsr, dhr, sizes, reduce)
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, H, W)
        assert torch.equal(got, _compose(dsr, dhr, sizes, reduce)), (sizes, reduce)
        assert torch.equal(got.cpu(), torch.from_numpy(multi_ref(sr, hr, sizes, reduce))), (sizes, reduce)
    assert torch.equal(M.error_maps_multi(dsr, dhr, [11], reduce), M.error_maps(dsr, dhr, 11))
    assert torch.equal(M.error_maps_multi(dsr, dhr, (4,)), M.error_maps(dsr, dhr, 4))            # reduce defaults to the mean


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C", [(33, 45, 1), (64, 64, 3)])
def test_a_list_of_one_size_is_the_single_map(H, W, C):
    """Window size 1 (no table), the smallest table window and the largest that fits, per-lane and scalar-row instance."""
    from srad_amd import metrics as M
    dsr, dhr = (_dev(a) for a in random_pairs(2, H, W, C, seed=21))
    for ws in (1, 2, 2 * min(H, W) - 1):
        single = M.error_maps(dsr, dhr, ws)
        for reduce in ("mean", "max"):
            assert torch.equal(M.error_maps_multi(dsr, dhr, [ws], reduce), single), (H, W, C, ws, reduce)


@pytest.mark.gpu
def test_batch_invariance():
    from srad_amd import metrics as M
    sr, hr = random_pairs(5, 64, 64, 3, seed=13)
    dsr, dhr = _dev(sr), _dev(hr)
    for ws in (1, 4, 11):
        whole = M.error_maps(dsr, dhr, ws)
        multi = M.error_maps_multi(dsr, dhr, [ws, 21], "mean")
        for k in range(5):
            assert torch.equal(whole[k:k + 1], M.error_maps(dsr[k:k + 1], dhr[k:k + 1], ws)), (ws, k)
            assert torch.equal(multi[k:k + 1], M.error_maps_multi(dsr[k:k + 1], dhr[k:k + 1], [ws, 21], "mean")), (ws, k)


@pytest.mark.gpu
def test_batch_invariance_across_a_chunk_boundary():
    """The table path works through the batch in chunks of ``score_plan``'s size (the SSIM map path's plan: 2^25 table points).
    At 256 x 256 a chunk holds 508 images, so 509 is the smallest batch that is split; the images on both sides of the split
    equal the same images in a small call, and the first ones too."""
    from srad_amd import metrics as M
    H = W = 256
    chunk = M.score_plan(10 ** 6, H, W)[1]
    assert chunk == (1 << 25) // ((H + 1) * (W + 1)) == 508
    n = chunk + 1
    assert M.score_plan(chunk, H, W)[1] == chunk and M.score_plan(n, H, W)[1] == chunk < n
    g = torch.Generator(device="cuda").manual_seed(3)
    hr = torch.randint(0, 256, (n, H, W, 1), generator=g, device="cuda", dtype=torch.uint8)
    sr = torch.randint(0, 256, (n, H, W, 1), generator=g, device="cuda", dtype=torch.uint8)
    whole = M.error_maps(sr, hr, 11)
    multi = M.error_maps_multi(sr, hr, [3, 11], "max")
    for a, b in ((0, 2), (chunk - 2, n)):
        assert torch.equal(whole[a:b], M.error_maps(sr[a:b].contiguous(), hr[a:b].contiguous(), 11)), (a, b)
        assert torch.equal(multi[a:b], M.error_maps_multi(sr[a:b].contiguous(), hr[a:b].contiguous(), [3, 11], "max")), (a, b)
    last = slice(n - 1, n)
    assert torch.equal(whole[last].cpu(), torch.from_numpy(error_map_ref(sr[last].cpu().numpy(), hr[last].cpu().numpy(), 11)))


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3])
def test_tie_to_the_image_score(C):
    """At ws 1 the float64 mean of an image's map is its MSE score up to the reference's fp32 rounding of a/255 and b/255: at most
    2 x 6e-8 absolute on a difference of at least 1/255 = 3e-5 relative on d, 6e-5 on d^2, plus the map's one fp32 rounding
    (6e-8 relative): within 1e-4 relative.  Every pixel of these pairs differs in every channel."""
    from srad_amd import metrics as M
    g = np.random.default_rng(17)
    hr = g.integers(0, 256, (4, 48, 40, C), dtype=np.uint8)
    step = g.integers(1, 255, hr.shape)                      # 1 .. 254 modulo 256: never zero
    sr = ((hr.astype(np.int64) + step) % 256).astype(np.uint8)
    assert np.all(sr != hr)
    dsr, dhr = _dev(sr), _dev(hr)
    mean = M.error_maps(dsr, dhr, 1).double().mean((1, 2)).cpu().numpy()
    _, mse, _ = M.score_pairs(dsr, dhr, [])
    mse = mse.cpu().numpy()
    rel = np.abs(mean - mse) / mse
    print("relative difference of the map mean to the MSE score:", rel)
    assert np.all(rel <= 1e-4), rel
    same = M.error_maps(dhr, dhr, 1)                         # identical images: both are exactly 0
    assert float(same.abs().max()) == 0.0 and float(M.score_pairs(dhr, dhr, [])[1].abs().max()) == 0.0


@pytest.mark.gpu
def test_errors():
    from srad_amd import metrics as M
    sr, hr = random_pairs(1, 33, 45, 1, seed=19)
    dsr, dhr = _dev(sr), _dev(hr)
    assert M.error_maps(dsr, dhr, 65).shape == (1, 33, 45)                          # the largest window that fits
    for ws in (66, 67, 0, -3):
        with pytest.raises(RuntimeError, match="error_maps: window .* needs more than one reflection of a 33x45"):
            M.error_maps(dsr, dhr, ws)
        with pytest.raises(RuntimeError, match="error_maps_multi: window .* needs more than one reflection"):
            M.error_maps_multi(dsr, dhr, [3, ws])
    with pytest.raises(RuntimeError, match="more than one reflection"):
        M.error_maps_multi(dsr, dhr, [3] * 17 + [67])        # in the second launch's part of the list: nothing runs
    with pytest.raises(ValueError, match="empty"):
        M.error_maps_multi(dsr, dhr, [])
    with pytest.raises(ValueError, match="reduce"):
        M.error_maps_multi(dsr, dhr, [3], reduce="sum")
    with pytest.raises(RuntimeError, match="GPU only"):
        M.error_maps(torch.from_numpy(sr), torch.from_numpy(hr), 3)

"""Shared test helpers: rebuild configs / synthetic state from a golden fixture entry."""
import numpy as np

from srad_amd import spec as S

DRN_GAIN = 0.5   # must match tests/golden/make_golden.py


def drct_case(g, name):
    in_chans, img_size, ws, upscale, n_rdg, seed = [int(v) for v in g[name + "/cfg"]]
    cfg = S.DRCTConfig(in_chans=in_chans, img_size=img_size, window_size=ws, upscale=upscale, n_rdg=n_rdg)
    sd = S.synth_state(S.drct_spec(cfg), seed=seed, gain=1.0, cfg=cfg)
    return cfg, sd, g[name + "/x"], g[name + "/y"]


def drn_case(g, name):
    n_colors, scale, seed = [int(v) for v in g[name + "/cfg"]]
    cfg = S.DRNConfig.for_scale(scale, n_colors)
    sd = S.synth_state(S.drn_spec(cfg), seed=seed, gain=DRN_GAIN, cfg=cfg)
    dual = S.synth_state(S.dual_spec(cfg), seed=seed + 100, gain=DRN_GAIN, cfg=cfg)
    ys = [g[f"{name}/y{j}"] for j in range(cfg.phase + 1)]
    return cfg, sd, dual, g[name + "/x"], ys, g[name + "/dual"]


DRCT_CASES = ["drct_full_gray_x4", "drct_r2_rgb_x4", "drct_r2_gray_x4_dyn64", "drct_r1_gray_x4_ws4",
              "drct_r1_gray_x8_ws2", "drct_r1_gray_x4_ws16"]
DRN_CASES = ["drn_x2_gray", "drn_x4_rgb", "drn_x4_gray", "drn_x8_gray"]


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- constructed tie groups for the sort-based pixel metrics (scan tile = 4096 keys, 16 per thread, 256 tiles per chunk) ----
# Group heads at sorted positions 0, 1, 16, 32, 49, 4095, 4096, 4097, 4098 and 8191; the group from 8191 runs past 20480, so scan
# tiles 2, 3 and 4 hold no head; a few short groups follow, and n = 20807 is no multiple of 16.
TIE_SMALL = [1, 15, 16, 17, 4046, 1, 1, 1, 4093, 12293, 2, 14, 300, 7]
TIE_CHUNK_N = 1031 * 1023


def tie_chunk_lengths():
    """n = 1031 * 1023 keys: lengths cycling 1..64 and one filler group up to key 255 * 4096 - 7, a group of 4096 + 32 keys from
    there (it crosses key 256 * 4096, where the one-block tile scan starts its second chunk, and tile 255 has no head), then
    groups of 5 and a last shorter one."""
    start = 255 * 4096 - 7
    lengths, total, k = [], 0, 0
    while start - total >= k % 64 + 1:
        lengths.append(k % 64 + 1)
        total += lengths[-1]
        k += 1
    if start > total:
        lengths.append(start - total)
    assert sum(lengths) == start and max(lengths) <= 64
    lengths.append(4096 + 32)
    rest = TIE_CHUNK_N - start - (4096 + 32)
    lengths += [5] * (rest // 5) + ([rest % 5] if rest % 5 else [])
    assert sum(lengths) == TIE_CHUNK_N
    return lengths


def pad_last_group(lengths, n):
    """The list with its last group lengthened so that the lengths add up to n."""
    assert n >= sum(lengths)
    return list(lengths[:-1]) + [lengths[-1] + n - sum(lengths)]


def tie_group_case(lengths, descending, seed):
    """Scores and labels whose sorted walk meets tie groups of exactly `lengths`, in that order: group j has the score j / 64 for
    an ascending walk, (G - j) / 64 for a descending one (exact in float32), labels are random at p = 0.37, and the whole is
    shuffled.  Returns (float32 scores, uint8 labels)."""
    G = len(lengths)
    assert G < (1 << 18)
    rng = np.random.default_rng(seed)
    j = np.repeat(np.arange(G), lengths)
    s = ((G - j) if descending else j).astype(np.float32) / np.float32(64)
    y = (rng.random(len(s)) < 0.37).astype(np.uint8)
    p = rng.permutation(len(s))
    return s[p], y[p]


# ---- the evaluator's post-sweep stage on the CPU: images, stand-ins for the map kernels, a gloo world-2 runner ----
N_IMG, HW, BEST_WS = 7, 24, 5           # images 0..2 are the good ones; BEST_WS: what rank 0's sweep is said to have found
Y_TRUE = [0, 0, 0] + [1] * (N_IMG - 3)
COLLECTIVES = ("all_gather_object", "broadcast_object_list", "all_reduce", "barrier", "gather_object", "broadcast", "all_gather")


def map_smooth_generator():
    """tests/golden/make_map_smooth_golden.py as a module (its numpy restatement of the Gaussian filter)."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_map_smooth_golden.py")
    spec = importlib.util.spec_from_file_location("make_map_smooth_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def stage_images(idx):
    """Deterministic u8 (sr, hr) stacks [n, HW, HW, 1] for image indices idx; the bad images (index >= 3) differ more."""
    import torch
    sr, hr = [], []
    for i in idx:
        y, x = np.mgrid[0:HW, 0:HW]
        h = ((y * 31 + x * 17 + i * 101) % 256).astype(np.uint8)
        d = ((y * 7 + x * 13 + i * 29) % (9 + 6 * i)).astype(np.int64)
        sr.append(np.clip(h.astype(np.int64) + d, 0, 255).astype(np.uint8)[:, :, None])
        hr.append(h[:, :, None])
    return torch.from_numpy(np.stack(sr)), torch.from_numpy(np.stack(hr))


def cpu_anomaly_maps(sr, hr, ws):
    return ((sr.float() - hr.float()).abs()[..., 0] / 255.0 * (1.0 + 0.1 * ws)).contiguous()


def cpu_error_maps(sr, hr, ws=1):
    d = sr.float() - hr.float()
    return ((d * d)[..., 0] / 65025.0 * (1.0 + 0.1 * ws)).contiguous()


def _cpu_multi(single, sr, hr, sizes, reduce):
    import torch
    acc = single(sr, hr, sizes[0])
    for ws in sizes[1:]:
        m = single(sr, hr, ws)
        acc = torch.maximum(acc, m) if reduce == "max" else acc + m
    return acc * float(np.float32(1.0 / len(sizes))) if reduce == "mean" else acc


def cpu_anomaly_maps_multi(sr, hr, sizes, reduce="mean"):
    return _cpu_multi(cpu_anomaly_maps, sr, hr, sizes, reduce)


def cpu_error_maps_multi(sr, hr, sizes, reduce="mean"):
    return _cpu_multi(cpu_error_maps, sr, hr, sizes, reduce)


def cpu_smooth_maps(maps, sigma, truncate=4.0, with_max=False):
    import torch
    out = torch.from_numpy(map_smooth_generator().smooth_ref(maps.numpy(), float(sigma), truncate))
    return (out, out.amax((1, 2))) if with_max else out


def must_not_be_called(name, why):
    def fn(*a, **k):
        raise AssertionError(f"{name} called {why}")
    return fn


MAP_STAND_INS = dict(anomaly_maps=cpu_anomaly_maps, anomaly_maps_multi=cpu_anomaly_maps_multi, error_maps=cpu_error_maps,
                     error_maps_multi=cpu_error_maps_multi, smooth_maps=cpu_smooth_maps)


class stand_ins:
    """Context: the evaluator module ``E`` with CPU stand-ins for the map kernels (``MAP_STAND_INS``, then ``metrics`` = further
    replacements by name on ``E.M``) and a ``save_anomaly_maps`` that appends (names, maps) to ``saved``; restored on exit."""

    def __init__(self, E, saved, **metrics):
        self.E, self.new = E, dict(MAP_STAND_INS, **metrics)
        self.save = lambda maps, names, splits, d: saved.append((list(names), maps.clone()))

    def __enter__(self):
        self.old = {k: getattr(self.E.M, k) for k in self.new}, self.E.save_anomaly_maps
        for k, fn in self.new.items():
            setattr(self.E.M, k, fn)
        self.E.save_anomaly_maps = self.save
        return self

    def __exit__(self, *exc):
        for k, fn in self.old[0].items():
            setattr(self.E.M, k, fn)
        self.E.save_anomaly_maps = self.old[1]


def stage_call(E, rank, world, map_ws=0, map_scales=(), map_reduce="mean", map_sigma=0.0, map_source=None, **asked):
    """The evaluator's post-sweep stage for rank ``rank`` of ``world`` on the images of ``stage_images``, without masks; only
    rank 0 knows the sweep's result.  ``asked``: save_maps, map_image_score, pixel_metrics, aupro."""
    mine = E.shard_indices(N_IMG, rank, world)
    sr, hr = stage_images(mine)
    shard = E.Shard(sr=sr, hr=hr, mine=mine, y_true=Y_TRUE, names=[f"im{i}" for i in range(N_IMG)], rank=rank, world=world,
                    output_dir="unused_dir")
    source = {} if map_source is None else dict(source=map_source)
    spec = E.MapSpec(ws=map_ws, scales=map_scales, reduce=map_reduce, sigma=map_sigma, **source).resolve(HW, HW)
    return E._pixel_stage(shard=shard, spec=spec, want=E.Request(**asked), masks=None, best_ws=BEST_WS if rank == 0 else None)


def _world2_rank(rank, world, port, q, job, args):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    for fn in COLLECTIVES:                                    # every collective call of this rank, by name, in order
        def counted(*a, _real=getattr(dist, fn), _fn=fn, **k):
            calls.append(_fn)
            return _real(*a, **k)
        setattr(dist, fn, counted)
    q.put((rank, job(rank, world, calls, *args)))
    dist.barrier()
    dist.destroy_process_group()


def run_world2(job, *args):
    """``job(rank, 2, calls, *args)`` (a module-level function) in two fresh gloo ranks; ``calls`` is the list the collective
    calls of that rank are appended to by name.  Returns {rank: what the job returned}."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_world2_rank, args=(r, 2, port, q, job, args)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in procs:
            r, out = q.get(timeout=240)
            res[r] = out
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert [p.exitcode for p in procs] == [0, 0]
    return res


def stage_sweep(E, rank, world, cases, calls=None, **metrics):
    """``stage_call`` for every flag set of ``cases`` under the stand-ins: [(result, the collective calls made, the saved
    (names, maps as numpy))] in the order of ``cases``."""
    saved, res = [], []
    with stand_ins(E, saved, **metrics):
        for flags in cases:
            del saved[:]
            if calls is not None:
                del calls[:]
            out = stage_call(E, rank, world, **flags)
            res.append((out, list(calls or ()), [(names, m.numpy()) for names, m in saved]))
    return res


def assert_saved_maps_complete(flags, f0, f1, wf):
    """With save_maps the two ranks' files are together the world-1 set, map for map; without, nobody wrote anything."""
    if not flags["save_maps"]:
        assert not f0 and not f1 and not wf
        return
    got = {n: m[j] for names, m in f0 + f1 for j, n in enumerate(names)}
    want = {n: m[j] for names, m in wf for j, n in enumerate(names)}
    assert sorted(got) == sorted(want) == [f"im{i}" for i in range(N_IMG)]
    for n in want:
        assert np.array_equal(got[n], want[n]), (flags, n)

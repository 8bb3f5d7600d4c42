"""Records which launches one DRCT training step runs: tests/golden/drct_train_census.json, the fixture of
tests/test_gpu_drct_train_census.py.  Needs a GPU.  Like make_drct_launch_census.py it is run at the commit whose launches are
the yardstick (recorded in the file, with the device name and its CU count), never on the code under test:

    python tests/golden/make_drct_train_census.py --commit <hash> [--out FILE] [--outputs FILE.npz]

A case is one 1-RDG model and one step on a fixed input, the smallest shape that reaches its Swin-block plan
(csrc/drct_train_plan.h).  Per case it keeps, between prof_enable / prof_collect and separately for the training forward and for
the backward, [launches, flops, bytes] per profiler class (flops and bytes are host-side sums over the launch parameters, so two
forms of a launch in one class still differ), what srad_drct_train_workspace_bytes answers for the shape, and wgrad_stats()
after the backward: the reduce launches by reason and the most floats a block had reserved.  --outputs also saves y, dx (where
the case asks for one) and the flat gradient of every case: what a change that promises the same bits is compared on."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "drct_train_census.json")

# name -> precision, input shape, window, upscale, img_size the mask buffers are built for, then the options:
#   keep   explicit DropPath factors through keep_scale_override (seeded)
#   build  path overrides held while the model is built and over the step;  step  over the step only
#   no_dx  the input does not require a gradient;  budget  the split-K workspace cut so that the largest block flushes mid-way
CASES = {
    "1_fp32_w8_2x16": ("fp32", (2, 1, 16, 16), 8, 2, 16, {}),
    "2_bf16_w8_2x16": ("bf16", (2, 1, 16, 16), 8, 2, 16, {}),
    "3_bf16_w8_2x16_droppath": ("bf16", (2, 1, 16, 16), 8, 2, 16, {"keep": True}),
    "4_bf16_unfused_build_and_step": ("bf16", (2, 1, 16, 16), 8, 2, 16, {"build": {"unfused_blocks": True}}),
    "5_bf16_unfused_step_only": ("bf16", (2, 1, 16, 16), 8, 2, 16, {"step": {"unfused_blocks": True}}),
    "6_bf16_w8_2x64_droppath": ("bf16", (2, 1, 64, 64), 8, 2, 64, {"keep": True}),
    "7_bf16_w16_1x32": ("bf16", (1, 1, 32, 32), 16, 2, 64, {}),
    "8_fp32_rgb_x4_no_dx": ("fp32", (2, 3, 16, 16), 8, 4, 16, {"no_dx": True}),
    "9_bf16_w8_2x16_budget_cut": ("bf16", (2, 1, 16, 16), 8, 2, 16, {"budget": True}),
}


def _model(precision, shape, window, upscale, img_size):
    from srad_amd import spec as S
    from srad_amd.nets import DRCT
    from tests.test_gpu_drct import Opt
    cfg = S.DRCTConfig(in_chans=shape[1], img_size=img_size, window_size=window, upscale=upscale, n_rdg=1)
    o = Opt(cfg, precision, False)
    o.drop_path_rate = 0.0
    m = DRCT(o)
    sd = {k: torch.from_numpy(S.synth_tensor(k, s, kind, seed=5, cfg=cfg)) for k, (s, kind) in S.drct_spec(cfg).items()
          if kind not in ("index", "mask")}
    m.load_state_dict(sd, strict=False)
    m = m.cuda().train()
    m.enable_training()
    return m, cfg


def _classes():
    from srad_amd import _lib as L
    return {k: [v["launches"], v["flops"], v["bytes"]] for k, v in sorted(L.prof_collect().items())}


def run_case(case, outputs=None):
    """The record of one case; with `outputs` a dict, y, dx (if asked for) and the flat gradient go into it as numpy arrays."""
    from srad_amd import _lib as L
    from srad_amd import ops
    precision, shape, window, upscale, img_size, opt = CASES[case]
    B, _, H, W = shape
    from srad_amd import spec as S
    x = torch.from_numpy(S.synth_image("census", shape, seed=3)).cuda()
    hr = torch.from_numpy(S.synth_image("census/hr", (B, shape[1], H * upscale, W * upscale), seed=4)).cuda()
    with ops.path_override(**opt.get("build", {})):
        m, cfg = _model(precision, shape, window, upscale, img_size)
        if opt.get("keep"):
            gen = torch.Generator().manual_seed(7)
            m.keep_scale_override = (torch.floor(0.7 + torch.rand(2 * cfg.n_rdg * 5, B, generator=gen)) / 0.7).cuda()

        def step(record):
            m.zero_grad()
            xt = x.clone().requires_grad_(not opt.get("no_dx"))
            rec = {}
            with ops.path_override(**opt.get("step", {})):
                L.prof_collect()
                y = m(xt)
                rec["forward"] = _classes()
                loss = F.l1_loss(y, hr)
                L.prof_collect()
                loss.backward()
                rec["backward"] = _classes()
            torch.cuda.synchronize()
            n, peak = m.wgrad_stats()
            rec["wgrad_stats"] = [n, peak]
            if record is not None:
                record["y"] = y.detach().cpu().numpy()
                record["flat_grad"] = m.flat_grads.cpu().numpy()
                if xt.grad is not None:
                    record["dx"] = xt.grad.cpu().numpy()
            return rec

        L.prof_enable(True)
        try:
            if opt.get("budget"):       # as test_gradients_do_not_depend_on_the_wgrad_budget: half a budget = the block peak less 1024 floats
                peak = step(None)["wgrad_stats"][1]
                m.set_wgrad_budget(2 * 4 * ((peak - 1024) // 128 * 128))
            rec = step(outputs)
        finally:
            L.prof_enable(False)
        nbytes = m._train_ws[(B, H, W)].numel() - 256         # what srad_drct_train_workspace_bytes answered for this shape
        rec["workspace_bytes"] = int(nbytes)
    return rec


def case_ids():
    return list(CASES)


def device_record():
    p = torch.cuda.get_device_properties(0)
    return {"device": p.name, "cus": int(p.multi_processor_count)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit this runs at (recorded)")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--outputs", default=None, help="also save y, dx and the flat gradient of every case: an .npz")
    a = ap.parse_args()
    doc = dict(device_record(), commit=a.commit, cases={})
    arrays = {}
    for case in case_ids():
        outs = {} if a.outputs else None
        doc["cases"][case] = run_case(case, outs)
        for k, v in (outs or {}).items():
            arrays[f"{case}#{k}"] = v
        print(case, "ok", flush=True)
    with open(a.out, "w") as f:                                  # one line per case
        head = {k: v for k, v in doc.items() if k != "cases"}
        f.write(json.dumps(head, sort_keys=True)[:-1] + ', "cases": {\n')
        f.write(",\n".join(f" {json.dumps(c)}: {json.dumps(r, sort_keys=True)}" for c, r in doc["cases"].items()))
        f.write("\n}}\n")
    if a.outputs:
        np.savez_compressed(a.outputs, **arrays)


if __name__ == "__main__":
    main()

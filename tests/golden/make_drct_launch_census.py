"""Records which launches the DRCT inference forward runs: tests/golden/drct_launch_census.json, the fixture of
tests/test_gpu_drct_launch_census.py.  Needs a GPU.  It is run at the commit whose launches are the yardstick (recorded in the
file, with the device name and its CU count: the chip-filling rules depend on it), never on the code under test:

    python tests/golden/make_drct_launch_census.py --commit <hash> [--out FILE]

A case is one 1-RDG model (precision x input) with the graph off.  Per override set it runs three forwards between
prof_enable / prof_collect and keeps, per profiler class, [launches, flops, bytes] of each (flops and bytes are host-side sums
over the launch parameters, so two forms of a launch in one class still differ):
  first   the first forward under this set - for the set "none" the first forward after build, fold builds and packs included
  second  the next forward: builds nothing
  third   the forward after layers.0.swin2.mlp.fc2.weight changed: that parameter's pack and exactly that block's rebuild
The per-call override sets share one model, in the order of CALL_SETS (so a fold that a set leaves stale is rebuilt in the first
forward of the next set that runs it, and "again" is one last forward with no override); unfused_blocks is read when the handle
is created and has a model of its own.  One more case binds a bf16 handle for training first: its folds stay off."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "drct_launch_census.json")

PRECISIONS = ["fp32", "bf16", "bf16x3"]
# name -> (input shape, window, upscale, img_size the mask buffers are built for, overrides held over the whole case)
INPUTS = {
    "w8_1x8": ((1, 1, 8, 8), 8, 4, 32, {}),
    "w8_2x16": ((2, 1, 16, 16), 8, 4, 32, {}),
    "w16_1x32": ((1, 1, 32, 32), 16, 4, 64, {}),
    "rgb_x2_1x8": ((1, 3, 8, 8), 8, 2, 32, {}),
    "w64_1x64": ((1, 1, 64, 64), 64, 4, 64, {}),
    "w64_1x64_qkv_via_gemm": ((1, 1, 64, 64), 64, 4, 64, {"qkv_via_gemm": True}),
}
FOUR = ("block_two_launches", "tail_chain", "ends_chain", "fc2_chain")
CALL_SETS = [("none", ())] + [(n, (n,)) for n in FOUR] + [("four_together", FOUR)]
CHANGED = "layers.0.swin2.mlp.fc2.weight"
TRAIN_BOUND = "bf16/w8_1x8/train_bound"


def _model(precision, name):
    from srad_amd import spec as S
    from tests.test_gpu_drct import Opt
    from srad_amd.nets import DRCT
    shape, window, upscale, img_size, _ = INPUTS[name]
    cfg = S.DRCTConfig(in_chans=shape[1], img_size=img_size, window_size=window, upscale=upscale, n_rdg=1)
    m = DRCT(Opt(cfg, precision, False))
    sd = {k: torch.from_numpy(S.synth_tensor(k, s, kind, seed=5, cfg=cfg)) for k, (s, kind) in S.drct_spec(cfg).items()
          if kind not in ("index", "mask")}
    m.load_state_dict(sd, strict=False)
    return m.cuda().eval()


def _three(m, x, outputs):
    from srad_amd import _lib as L
    rec = {}
    for which in ("first", "second", "third"):
        if which == "third":
            m.get_parameter(CHANGED).mul_(1.25)
        L.prof_collect()
        y = m(x)
        prof = L.prof_collect()
        rec[which] = {k: [v["launches"], v["flops"], v["bytes"]] for k, v in sorted(prof.items())}
        if outputs is not None:
            outputs.append(y.cpu().numpy())
    return rec


def census(precision, name, outputs=None):
    """{override set: {first / second / third: {class: [launches, flops, bytes]}}} of one (precision, input); with `outputs` a
    list, every forward's image is appended to it in order."""
    from srad_amd import _lib as L
    from srad_amd import ops
    shape, held = INPUTS[name][0], INPUTS[name][-1]
    x = torch.rand(shape, generator=torch.Generator().manual_seed(sum(shape))).cuda()
    out = {}
    L.prof_enable(True)
    try:
        with torch.no_grad(), ops.path_override(**held):
            m = _model(precision, name)
            for label, names in CALL_SETS:
                with ops.path_override(**{n: True for n in names}):
                    out[label] = _three(m, x, outputs)
            L.prof_collect()
            y = m(x)
            out["again"] = {"first": {k: [v["launches"], v["flops"], v["bytes"]] for k, v in sorted(L.prof_collect().items())}}
            if outputs is not None:
                outputs.append(y.cpu().numpy())
            del m
            with ops.path_override(unfused_blocks=True):
                out["unfused_blocks"] = _three(_model(precision, name), x, outputs)
    finally:
        L.prof_enable(False)
    return out


def census_train_bound(outputs=None):
    """A bf16 handle bound for training, then three inference forwards"""
    from srad_amd import _lib as L
    name = "w8_1x8"
    shape = INPUTS[name][0]
    x = torch.rand(shape, generator=torch.Generator().manual_seed(sum(shape))).cuda()
    m = _model("bf16", name)
    m.enable_training()
    m.eval()
    L.prof_enable(True)
    try:
        with torch.no_grad():
            return {"none": _three(m, x, outputs)}
    finally:
        L.prof_enable(False)


def case_ids():
    return [f"{p}/{n}" for p in PRECISIONS for n in INPUTS] + [TRAIN_BOUND]


def run_case(case, outputs=None):
    if case == TRAIN_BOUND:
        return census_train_bound(outputs)
    precision, name = case.split("/")
    return census(precision, name, outputs)


def device_record():
    p = torch.cuda.get_device_properties(0)
    return {"device": p.name, "cus": int(p.multi_processor_count)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit this runs at (recorded)")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--outputs", default=None, help="also save every forward's image: an .npz, one array per case and forward")
    a = ap.parse_args()
    doc = dict(device_record(), commit=a.commit, cases={})
    images = {}
    for case in case_ids():
        outs = [] if a.outputs else None
        doc["cases"][case] = run_case(case, outs)
        for i, y in enumerate(outs or []):
            images[f"{case}#{i}"] = y
        print(case, "ok", flush=True)
    with open(a.out, "w") as f:                                  # one line per case
        head = {k: v for k, v in doc.items() if k != "cases"}
        f.write(json.dumps(head, sort_keys=True)[:-1] + ', "cases": {\n')
        f.write(",\n".join(f" {json.dumps(c)}: {json.dumps(r, sort_keys=True)}" for c, r in doc["cases"].items()))
        f.write("\n}}\n")
    if a.outputs:
        np.savez_compressed(a.outputs, **images)


if __name__ == "__main__":
    main()

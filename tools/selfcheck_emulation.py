#!/usr/bin/env python3
"""CPU only: how good an estimate of e16 = max |fp16 storage - fp32| is the self-check's storage_err = max |fp16 storage - precise|?
For each stand-in model a 148 x 148 tile goes through the fp32 oracle and through tests/torch_ref.py's emulation of the engine's two
storages (trunk="fp16" / trunk="split", fea16=False, out32=True).  Two tiles: the padded tile of the C1 frame
(synth.make_image(1234, 256, 256), as profiles/r05_fp16_storage.txt) and the self-check's built-in tile (rsr_selfcheck_tile).
    python tools/selfcheck_emulation.py [model=i] [tile=photo|builtin]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch_ref  # noqa: E402
import oracle  # noqa: E402
import realsr_ncnn_vulkan_amd as R  # noqa: E402
from realsr_ncnn_vulkan_amd import synth  # noqa: E402

MODELS = [
    ("42", 42, {}),
    ("43", 43, {}),
    ("44 hot=32 last_gain=0.15", 44, {"hot": 32.0, "last_gain": 0.15}),
    ("45 chan_sigma=1 last_gain=0.12", 45, {"chan_sigma": 1.0, "last_gain": 0.12}),
    ("45 chan_sigma=1 last_gain=0.2 (wide)", 45, {"chan_sigma": 1.0, "last_gain": 0.2}),
]


def tiles():
    img = synth.make_image(1234, 256, 256)
    big = np.pad(img, ((10, 10), (10, 10), (0, 0)), mode="reflect")
    photo = np.ascontiguousarray(big[:148, :148, :3].astype(np.float32).transpose(2, 0, 1) * np.float32(1 / 255.0))
    return {"photo": photo, "builtin": R.selfcheck_tile(148, 148).astype(np.float32)}


def main():
    only, which = None, None
    for a in sys.argv[1:]:
        k, v = a.split("=")
        if k == "model":
            only = int(v)
        if k == "tile":
            which = v
    print("# emulated storages vs the fp32 oracle, 148 x 148 tile, [0,1] units; headroom = (1/255) / error")
    for tname, t in tiles().items():
        if which is not None and which != tname:
            continue
        for mi, (name, seed, kw) in enumerate(MODELS):
            if only is not None and only != mi:
                continue
            d = synth.make_model_dir("/tmp/rsr_models_probe", "m_%d_%s" % (seed, "_".join("%s%g" % kv for kv in sorted(kw.items()))), seed, **kw)
            pp, bp = os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")
            net = oracle.OracleNet(pp, bp)
            weights = [(c["weight"], c["bias"]) for c in (net.conv(i) for i in range(net.num_convs))]
            ref = net.forward(t)
            a16 = torch_ref.net_forward_storage_np(weights, t, trunk="fp16")
            aP = torch_ref.net_forward_storage_np(weights, t, trunk="split", fea16=False, out32=True)
            e16, eP, est = np.abs(a16 - ref).max(), np.abs(aP - ref).max(), np.abs(a16 - aP).max()
            print("%-8s model %-38s e16 %.3e (%.2f)  eP %.3e  storage_err %.3e (est. headroom %.2f)  est/e16 %.2f" % (
                tname, name, e16, (1 / 255) / e16, eP, est, (1 / 255) / est, est / e16))
            sys.stdout.flush()


if __name__ == "__main__":
    main()

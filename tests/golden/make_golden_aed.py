#!/usr/bin/env python3
"""Golden vectors of the AED detector (Darknet-21 + YOLOPAFPN + YOLOXHead at [256, 256, 256]: the ``basic`` / ``taf`` /
``taf_bfm`` recipes, core/exp.py:352-384,393-470), produced by the REFERENCE's own modules on torch-CPU fp32 with recipe
weights.  Stubs, input and labels are those of make_golden_detector.py (imported, not copied).

Runs only where the reference tree is available (FRLW_REFERENCE).  Weights are not stored: recipe_state_dict regenerates them
from (seed, parameter name) on both sides; the inputs are regenerated from their seeds.

    python tests/golden/make_golden_aed.py     # rewrites tests/golden/detector_aed.npz
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_detector import Focus, RefModel, YOLOPAFPN, YOLOXHead, detector_input, train_labels  # noqa: E402  (stubs first)

from core.Others.Temporal_Active_Focus import Temporal_Active_Focus_connect  # noqa: E402
from core.yolox.models.darknet import Darknet  # noqa: E402

from frlw_evd_amd.yolox.model import build_aed, recipe_state_dict  # noqa: E402

TAGS = (("aed_ev10", 10, "focus"), ("aed_eci4", 4, "focus"), ("aed_taf16", 16, "focus"), ("aed_bfm8", 8, "bfm"))
CHANS = [256, 256, 256]


def reference_aed(C, nc, stem):
    """core/exp.py:369,372,384 with the values of configModel (:359-365); radius 5 = gen1."""
    layer = Temporal_Active_Focus_connect if stem == "bfm" else Focus
    return RefModel(Darknet(21, (256, 320), layer, in_channels=C, out_features=["dark3", "dark4", "dark5"], act="silu",
                            out_channels=CHANS, stem_out_channels=64),
                    YOLOPAFPN(0.33, in_features=["dark3", "dark4", "dark5"], in_channels=CHANS, act="silu"), None,
                    YOLOXHead(nc, in_channels=CHANS, act="silu", strides=[8, 16, 32], radius=5))


def stats(t):
    return np.array([t.mean().item(), t.norm().item(), t.abs().max().item()])


def main():
    out = {}
    for tag, C, stem in TAGS:
        nc = 2
        ref = reference_aed(C, nc, stem)
        mine = build_aed(C, nc, stem=stem)
        sd = recipe_state_dict(mine, seed=1004)
        assert list(sd.keys()) == list(ref.state_dict().keys()), "parameter names differ from the reference"
        for (k, a), (_, b) in zip(sd.items(), ref.state_dict().items()):
            assert a.shape == b.shape, k
        ref.load_state_dict(sd)
        ref.eval()
        x = detector_input(1004, 2, C)
        with torch.no_grad():
            stem_out = ref.backbone.stem(x[..., 0])
            feats = ref.backbone(x[..., 0])
            fpn = ref.neck(feats)
            head = ref.head
            head.decode_in_inference = False
            raw = head(fpn)  # (B, 1680, 5 + nc) pre-decode
        out[f"{tag}_raw"] = raw.numpy()
        for name, t in zip(("dark3", "dark4", "dark5"), feats):
            out[f"{tag}_{name}_stats"] = stats(t)
        for name, t in zip(("pan2", "pan1", "pan0"), fpn):
            out[f"{tag}_{name}_stats"] = stats(t)
        out[f"{tag}_stem_crop"] = stem_out[:, :, 40:48, 100:108].numpy()   # (2, 64, 8, 8)
        out[f"{tag}_params"] = np.array(sum(p.numel() for p in ref.parameters()))
        # the reference's own state_dict: names and shapes, in order
        out[f"{tag}_keys"] = np.array(json.dumps([[k, list(v.shape)] for k, v in ref.state_dict().items()]))
        # decoded (pre-NMS) boxes with the reference's own arithmetic (yolo_head.py:258-272)
        grids, strides = [], []
        for (h, w), s in zip(head.hw, head.strides):
            yv, xv = torch.meshgrid([torch.arange(h), torch.arange(w)])
            grids.append(torch.stack((xv, yv), 2).view(1, -1, 2))
            strides.append(torch.full((1, h * w, 1), s))
        grids = torch.cat(grids, 1).float()
        strides = torch.cat(strides, 1).float()
        dec = raw.clone()
        dec[..., :2] = (dec[..., :2] + grids) * strides
        dec[..., 2:4] = torch.square(dec[..., 2:4]) * strides
        out[f"{tag}_decoded"] = dec.numpy()
        if tag == "aed_ev10":
            # train branch: SimOTA + losses + backward on a fixed label set (yolo_head.py:305-473)
            ref.load_state_dict(sd)
            ref.train()
            ref.head.decode_in_inference = True
            xt = detector_input(1005, 4, C)
            labels = train_labels()
            loss = ref(xt, labels, None, None)          # core/model.py:50-56 returns losses[0]
            out["aed_train_loss"] = np.array(loss.item())
            ref.zero_grad()
            loss.backward()
            for grp in ("backbone", "neck", "head"):
                out[f"aed_train_gradnorm_{grp}"] = np.array(float(torch.sqrt(sum(
                    (p.grad.double() ** 2).sum() for n, p in ref.named_parameters() if n.startswith(grp) and p.grad is not None))))
            feats = ref.neck(ref.backbone(xt[..., 0, 0][..., None]))
            tup = ref.head(feats, labels, xt[..., 0])
            out["aed_train_tuple"] = np.array([float(v) for v in tup])
    path = os.path.join(HERE, "detector_aed.npz")
    np.savez_compressed(path, **out)
    print("detector_aed.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()

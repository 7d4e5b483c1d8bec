"""The AED detector (Darknet-21 + YOLOPAFPN + YOLOXHead, 256 wide: the ``basic`` / ``taf`` / ``taf_bfm`` recipes) as plain
PyTorch on the CPU against golden vectors the REFERENCE's own modules produced (tests/golden/make_golden_aed.py), the recipe
dispatch of the entry points, and the plan of the ``yolox`` recipe, which adding a second backbone must not move."""
import json
import os

import numpy as np
import pytest
import torch

from frlw_evd_amd.yolox.model import build_aed, build_yolox, recipe_state_dict

TAGS = [("aed_ev10", 10, "focus", 14_823_445), ("aed_eci4", 4, "focus", 14_809_621), ("aed_taf16", 16, "focus", 14_837_269),
        ("aed_bfm8", 8, "bfm", 14_819_477)]  # the reference's own parameter counts


def detector_input(seed, B, C=10, H=256, W=320):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, 256, size=(B, C, H, W, 1, 1)).astype(np.float32) / np.float32(255))


def train_labels():
    lab = torch.zeros((4, 80, 5), dtype=torch.float64)
    lab[0, 0] = torch.tensor([1, 100.0, 120.0, 40.0, 60.0])
    lab[0, 1] = torch.tensor([0, 200.0, 80.0, 30.0, 30.0])
    lab[1, 0] = torch.tensor([0, 160.0, 128.0, 80.0, 50.0])
    lab[2, 0] = torch.tensor([1, 30.5, 40.25, 21.0, 33.0])
    lab[2, 1] = torch.tensor([1, 36.0, 44.0, 25.0, 30.0])
    lab[2, 2] = torch.tensor([0, 290.0, 230.0, 50.0, 40.0])
    return lab


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "detector_aed.npz"))


@pytest.mark.parametrize("tag,C,stem,n_params", TAGS)
def test_state_dict_is_the_references(golden, tag, C, stem, n_params):
    """Same names, order and shapes as the reference's model (checkpoints interchange), same parameter count."""
    m = build_aed(C, 2, stem=stem)
    want = json.loads(str(golden[f"{tag}_keys"]))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want
    assert "backbone.dark3.1.layer2.conv.weight" in m.state_dict() and "backbone.dark5.4.conv2.bn.weight" in m.state_dict()
    assert sum(p.numel() for p in m.parameters()) == int(golden[f"{tag}_params"]) == n_params


@pytest.mark.parametrize("tag,C,stem,n_params", TAGS)
def test_eager_matches_reference(golden, tag, C, stem, n_params):
    """The rule of tests/test_detector_cpu.py: same ops on the same weights, only the CPU backend's summation order may differ."""
    torch.set_num_threads(8)
    m = build_aed(C, 2, stem=stem)
    m.load_state_dict(recipe_state_dict(m, seed=1004))
    m.eval()
    x = detector_input(1004, 2, C)
    with torch.no_grad():
        stem_out = m.backbone.stem(x[..., 0])
        feats = m.backbone(x[..., 0])
        fpn = m.neck(feats)
        raw = m.reference_outputs(x[..., 0])
    crop = golden[f"{tag}_stem_crop"]
    assert np.abs(stem_out[:, :, 40:48, 100:108].numpy() - crop).max() <= 1e-5 * np.abs(crop).max()
    for name, t in zip(("dark3", "dark4", "dark5", "pan2", "pan1", "pan0"), list(feats) + list(fpn)):
        # the same rule on the summaries: an element-wise error of e = 1e-5 |max| moves the mean and the |max| by at most e
        # and the norm by at most e sqrt(N)
        mean, norm, amax = golden[f"{tag}_{name}_stats"]
        e = 1e-5 * amax
        assert abs(t.mean().item() - mean) <= e and abs(t.abs().max().item() - amax) <= e, name
        assert abs(t.norm().item() - norm) <= e * t.numel() ** 0.5, name
    want = golden[f"{tag}_raw"]
    assert raw.shape == (2, 1680, 7)
    assert np.abs(raw.numpy() - want).max() <= 1e-5 * np.abs(want).max()
    dec = m.head.decode_boxes(raw)
    assert np.abs(dec.numpy() - golden[f"{tag}_decoded"]).max() <= 1e-4


def test_train_branch_matches_reference(golden):
    """SimOTA assignment + losses + backward through Darknet-21 against the reference's own numbers."""
    torch.set_num_threads(8)
    m = build_aed(10, 2)
    m.load_state_dict(recipe_state_dict(m, seed=1004))
    m.train()
    x = detector_input(1005, 4)
    labels = train_labels()
    loss = m(x, labels, None, None)
    assert float(loss) == pytest.approx(float(golden["aed_train_loss"]), rel=1e-6)
    loss.backward()
    for grp in ("backbone", "neck", "head"):
        gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for n, p in m.named_parameters() if n.startswith(grp))))
        assert gn == pytest.approx(float(golden[f"aed_train_gradnorm_{grp}"]), rel=1e-4), grp
    tup = m.head(m.neck(m.backbone(x[..., 0])), labels, x[..., 0])
    assert [float(v) for v in tup] == pytest.approx(list(golden["aed_train_tuple"]), rel=1e-5)


def test_pick_experiment_knows_the_aed_recipes():
    import train as train_entry
    from frlw_evd_amd import exp
    assert train_entry.pick_experiment("basic") is exp.basicExp
    assert train_entry.pick_experiment("taf") is exp.tafExp
    assert train_entry.pick_experiment("taf_bfm") is exp.tafBFMExp
    assert issubclass(exp.tafBFMExp, exp.tafExp) and issubclass(exp.tafExp, exp.basicExp)  # core/exp.py:393,467
    for name in ("yolov3", "yolov3_taf_bfm"):
        with pytest.raises(SystemExit):
            train_entry.pick_experiment(name)


@pytest.mark.parametrize("name,bins,dataset,n_params,radius", [("basic", 5, "gen1", 14_823_445, 5), ("taf", 8, "gen4", None, 2.5),
                                                              ("taf_bfm", 4, "gen1", 14_819_477, 5)])
def test_recipes_build_the_aed_model(name, bins, dataset, n_params, radius):
    """configModel .. buildHead of the three recipes (core/exp.py:352-384,467-470): Darknet-21, 256-wide neck and head, the BFM
    stem for taf_bfm, radius 5 for gen1 and 2.5 otherwise."""
    import types
    from frlw_evd_amd import exp
    from frlw_evd_amd.yolox.darknet import Darknet
    settings = types.SimpleNamespace(event_volume_bins=bins, dataset_name=dataset, img_size=[256, 320], local_rank=0, synthetic=True)
    e = exp.EXPERIMENTS[name](settings)
    e.object_classes = exp.GEN1_CLASSES if dataset == "gen1" else exp.GEN4_CLASSES
    e.configModel(); e.buildBackbone(); e.buildNeck(); e.buildMemory(); e.buildHead()
    assert isinstance(e.backbone, Darknet) and e.neck.in_channels == [256, 256, 256] and e.head.radius == radius
    assert hasattr(e.backbone.stem, "trans_up") == (name == "taf_bfm")
    assert e.backbone.stem.conv.conv.in_channels == (4 * 8 if name == "taf_bfm" else 8 * bins)
    if n_params is not None:
        n = sum(p.numel() for m in (e.backbone, e.neck, e.head) for p in m.parameters())
        assert n == n_params


# ops_meta of the yolox plan at (10, 256, 320), float32, as the commit before the Darknet builder produced it
YOLOX_OPS = [
    ('fstem', 20480, 32, 360, 471859200), ('conv', 5120, 64, 288, 188743680), ('conv', 5120, 64, 64, 41943040),
    ('conv', 5120, 32, 32, 10485760), ('conv', 5120, 32, 288, 94371840), ('conv', 5120, 64, 64, 41943040),
    ('conv', 1280, 128, 576, 188743680), ('conv', 1280, 128, 128, 41943040), ('conv', 1280, 64, 64, 10485760),
    ('conv', 1280, 64, 576, 94371840), ('conv', 1280, 64, 64, 10485760), ('conv', 1280, 64, 576, 94371840),
    ('conv', 1280, 64, 64, 10485760), ('conv', 1280, 64, 576, 94371840), ('conv', 1280, 128, 128, 41943040),
    ('conv', 320, 256, 1152, 188743680), ('conv', 320, 256, 256, 41943040), ('conv', 320, 128, 128, 10485760),
    ('conv', 320, 128, 1152, 94371840), ('conv', 320, 128, 128, 10485760), ('conv', 320, 128, 1152, 94371840),
    ('conv', 320, 128, 128, 10485760), ('conv', 320, 128, 1152, 94371840), ('conv', 320, 256, 256, 41943040),
    ('conv', 80, 512, 2304, 188743680), ('conv', 80, 256, 512, 20971520), ('spp', 80, 256, 0, 0),
    ('conv', 80, 512, 1024, 83886080), ('conv', 80, 512, 512, 41943040), ('conv', 80, 256, 256, 10485760),
    ('conv', 80, 256, 2304, 94371840), ('conv', 80, 512, 512, 41943040), ('conv', 80, 256, 512, 20971520),
    ('conv', 320, 256, 512, 83886080), ('conv', 320, 128, 128, 10485760), ('conv', 320, 128, 1152, 94371840),
    ('conv', 320, 256, 256, 41943040), ('conv', 320, 128, 256, 20971520), ('conv', 1280, 128, 256, 83886080),
    ('conv', 1280, 64, 64, 10485760), ('conv', 1280, 64, 576, 94371840), ('conv', 1280, 128, 128, 41943040),
    ('conv', 320, 128, 1152, 94371840), ('conv', 320, 256, 256, 41943040), ('conv', 320, 128, 128, 10485760),
    ('conv', 320, 128, 1152, 94371840), ('conv', 320, 256, 256, 41943040), ('conv', 80, 256, 2304, 94371840),
    ('conv', 80, 512, 512, 41943040), ('conv', 80, 256, 256, 10485760), ('conv', 80, 256, 2304, 94371840),
    ('conv', 80, 512, 512, 41943040), ('conv', 1280, 256, 128, 83886080), ('conv', 1280, 256, 2304, 1509949440),
    ('conv', 1280, 256, 2304, 1509949440), ('conv', 1280, 256, 2304, 1509949440), ('conv', 1280, 256, 2304, 1509949440),
    ('conv', 320, 256, 256, 41943040), ('conv', 320, 512, 2304, 754974720), ('conv', 320, 512, 2304, 754974720),
    ('conv', 80, 256, 512, 20971520), ('conv', 80, 512, 2304, 188743680), ('conv', 80, 512, 2304, 188743680),
    ('pred', 1680, 7, 512, 6021120)
]


def test_yolox_plan_is_unchanged():
    from frlw_evd_amd.detector import DetectorEngine
    net = build_yolox(10, 2).eval()
    e = DetectorEngine(net, device="cpu", precision="f32")  # (a plan on "cpu" is never run: its op list is what is read)
    e.build((10, 256, 320))
    assert e.ops_meta == YOLOX_OPS
    assert (e.n_forward_ops, e.n_conv, e.flops_per_image) == (66, 62, 11655700480)


def test_aed_plans():
    """The AED plans: one fused Focus + stem op where the kernel takes the shape (C in {4, 8, 10, 16}), Focus and a convolution
    elsewhere; 16.3 GFLOP per 256 x 320 x 10 image."""
    from frlw_evd_amd.detector import DetectorEngine
    for C, stem, first in ((10, "focus", ["fstem"]), (4, "focus", ["fstem"]), (16, "focus", ["fstem"]), (6, "focus", ["focus", "conv"]),
                           (8, "bfm", ["bfm", "conv"])):
        e = DetectorEngine(build_aed(C, 2, stem=stem).eval(), device="cpu", precision="f32")
        e.build((C, 256, 320))
        kinds = [o[0] for o in e.ops_meta]
        assert kinds[:len(first)] == first and kinds.count("spp") == 1 and kinds[-1] == "pred", (C, stem, kinds)
        assert ("focus" in kinds) == (first[0] == "focus") and kinds.count("fstem") == (first[0] == "fstem")
        assert e.ops_meta[len(first) - 1][2] == 64  # the stem is 64 wide
        if C == 10:
            assert e.flops_per_image == pytest.approx(16.27e9, rel=1e-3)

"""Evaluation straight from recordings, the parts that need no GPU: representation names, the planned sample lists against the
commands' own slicers, the ``test.py`` flags and settings, the numpy restatement of the hand-off against the oracle's resize, the
library export, and that the entry-point cases of tests/test_recording_eval_gpu.py are about real boxes (CPU forward of the
oracle's volumes)."""
import os
import sys
import types

import numpy as np
import pytest

import hand_off_restated as restated
import recording_eval_data as red

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

README_NAMES = {   # DATA_DIR names of the README's tables, per dataset
    "gen1": ["taf", "EventVolume250000", "EventVolume500000", "EventVolume1000000", "EventCountImage50000", "EventCountImage100000",
             "EventCountImage200000", "SurfaceOfActiveEvents0.00001", "SurfaceOfActiveEvents0.0000025", "SurfaceOfActiveEvents0.000001"],
    "gen4": ["taf", "EventVolume250000", "EventVolume500000", "EventVolume1000000", "EventCountImage400000", "EventCountImage800000",
             "EventCountImage1200000", "SurfaceOfActiveEvents0.00001", "SurfaceOfActiveEvents0.0000025", "SurfaceOfActiveEvents0.000001"],
}


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return red.build_dataset(str(tmp_path_factory.mktemp("recording_eval")))


def test_parse_representation_takes_every_readme_name():
    from frlw_evd_amd import generate
    from frlw_evd_amd.recording_dataset import parse_representation
    for ds, names in README_NAMES.items():
        kinds = [parse_representation(n, ds) for n in names]
        assert [k for k, _ in kinds] == ["taf"] + ["ev"] * 3 + ["eci"] * 3 + ["sae"] * 3
        assert [p for _, p in kinds] == [None] + generate.EV_TIME_WINDOWS + generate.eci_events_windows(ds) + generate.SAE_LAMDAS
    # the directory names the SAE command itself writes (str(float))
    assert parse_representation("SurfaceOfActiveEvents1e-05", "gen1") == ("sae", 0.00001)
    assert parse_representation("SurfaceOfActiveEvents2.5e-06", "gen4") == ("sae", 0.0000025)


@pytest.mark.parametrize("name,ds", [("TAF", "gen1"), ("", "gen1"), ("bins8", "gen1"), ("EventVolume", "gen1"), ("EventVolume250001", "gen1"),
                                     ("EventVolume0250000", "gen1"), ("EventVolume250000x", "gen1"), ("EventCountImage400000", "gen1"),
                                     ("EventCountImage50000", "gen4"), ("EventCountImage-50000", "gen1"),
                                     ("SurfaceOfActiveEvents0.001", "gen1"), ("SurfaceOfActiveEventsnan", "gen1"),
                                     ("SurfaceOfActiveEvents", "gen4"), ("EventFrame", "gen1")])
def test_parse_representation_refuses_what_no_command_writes(name, ds):
    from frlw_evd_amd.recording_dataset import parse_representation
    with pytest.raises(ValueError):
        parse_representation(name, ds)


def test_event_volume_bins_must_fit_the_kind():
    from frlw_evd_amd.recording_dataset import parse_representation, representation_channels
    fits = {"taf": [8, 4], "EventVolume250000": [5], "EventCountImage50000": [1], "SurfaceOfActiveEvents0.000001": [1]}
    for name, good in fits.items():
        kind, _ = parse_representation(name, "gen1")
        for bins in range(0, 10):
            if bins in good:
                assert parse_representation(name, "gen1", bins)[0] == kind and representation_channels(kind, bins) == 2 * bins
            else:
                with pytest.raises(ValueError, match=f"--event_volume_bins {good[0]}"):
                    parse_representation(name, "gen1", bins)


@pytest.mark.parametrize("name,bins,kind", [("taf", 8, "taf"), ("EventVolume500000", 5, "ev"), ("EventCountImage100000", 1, "eci"),
                                            ("SurfaceOfActiveEvents0.0000025", 1, "sae")])
def test_planned_samples_are_the_files_the_command_names(dataset, name, bins, kind):
    """Host code only (the device is never touched: ``device="cpu"`` would not even encode)."""
    from frlw_evd_amd.recording_dataset import RecordingLoader
    raw, lab = dataset
    want = red.planned_samples(raw, lab, kind)
    loader = RecordingLoader(lab, raw, name, "gen1", [256, 320], [256, 320], bins, "test", 4, "cpu")
    assert loader.samples == want
    assert sorted(red.split_sequences(lab)) == ["seqA", "seqB"]
    # seqA's label at 7.3 s lies behind its last event: skipped (Event Volume: it ends the file's loop -- it is the last label)
    assert len(want) == 9 and ("seqA", 7_300_000) not in want and ("seqA", 603_000) in want and ("seqB", 1_400_000) in want
    assert len(loader) == 3 and (loader.width, loader.height) == (304, 240) and loader.object_classes == ["Car", "Pedestrian"]
    assert len(RecordingLoader(lab, raw, name, "gen1", [256, 320], [256, 320], bins, "test", 9, "cpu")) == 1


def test_loader_arguments(dataset):
    from frlw_evd_amd.recording_dataset import RecordingLoader
    raw, lab = dataset
    with pytest.raises(ValueError, match="--event_volume_bins 5"):
        RecordingLoader(lab, raw, "EventVolume250000", "gen1", [256, 320], [256, 320], 8, "test", 4, "cpu")
    with pytest.raises(ValueError):
        RecordingLoader(lab, raw, "EventCountImage400000", "gen1", [256, 320], [256, 320], 1, "test", 4, "cpu")
    with pytest.raises(ValueError):
        RecordingLoader(lab, raw, "taf", "gen1", [256, 320], [256, 320], 8, "test", 65, "cpu")
    with pytest.raises(ValueError):
        RecordingLoader(lab, raw, "taf", "gen1", [512, 640], [512, 640], 8, "test", 4, "cpu")


def test_command_line_flags():
    import test as test_entry
    a = test_entry.parse_args("--raw_dir R --representation taf --exp_type yolox_taf_bfm --event_volume_bins 4".split())
    assert (a.raw_dir, a.representation, a.bbox_path, a.data_path) == ("R", "taf", "R", None)   # the README keeps both in one tree
    a = test_entry.parse_args("--raw_dir R --bbox_path B --representation EventVolume250000".split())
    assert (a.raw_dir, a.bbox_path) == ("R", "B")
    a = test_entry.parse_args("--bbox_path B --data_path D".split())
    assert (a.raw_dir, a.representation, a.data_path) == (None, None, "D")
    for bad in ("--raw_dir R --data_path D --representation taf", "--raw_dir R", "--data_path D --bbox_path B --representation taf"):
        with pytest.raises(SystemExit):
            test_entry.parse_args(bad.split())


def test_settings_carry_the_route(tmp_path):
    import test as test_entry
    import train as train_entry
    from frlw_evd_amd.settings import Setting_test
    base = dict(local_rank=0, resume_exp=None, exp_type="yolox", log_path=str(tmp_path) + "/", record=None, dataset="gen1", bbox_path="B",
                data_path="D", event_volume_bins=5, batch_size=1, num_cpu_workers=2, nodes=1)
    st = Setting_test(types.SimpleNamespace(**base))           # a parser without the new flags
    assert st.raw_dir is None and st.representation is None and not st.synthetic
    args = test_entry.parse_args(["--raw_dir", "R", "--representation", "EventVolume250000", "--log_path", str(tmp_path) + "/"])
    args.local_rank = 0
    st = Setting_test(args)
    assert (st.raw_dir, st.representation, st.bbox_path, st.data_path) == ("R", "EventVolume250000", "R", None) and not st.synthetic
    assert not any(o in ("--raw_dir", "--representation") for a in train_entry.build_parser()._actions for o in a.option_strings)


@pytest.mark.parametrize("exp_name,bins,representation,fitting", [
    ("yolox", 5, "taf", "EventVolume"), ("basicExp", 1, "taf", "EventCountImage"), ("yoloxtafBFM", 4, "EventVolume250000", "taf"),
    ("tafExp", 8, "SurfaceOfActiveEvents0.00001", "taf"), ("tafBFMExp", 8, "EventCountImage50000", "taf")])
def test_representation_must_fit_the_experiment(dataset, exp_name, bins, representation, fitting):
    from frlw_evd_amd import exp
    raw, lab = dataset
    settings = types.SimpleNamespace(event_volume_bins=bins, dataset_name="gen1", img_size=[256, 320], input_img_size=[256, 320],
                                     raw_dir=raw, bbox_path=lab, data_path=None, representation=representation, batch_size=4,
                                     gpu_device=torch.device("cpu"), synthetic=False)
    with pytest.raises(SystemExit, match=fitting):
        getattr(exp, exp_name)(settings)._disk_loaders(test_only=True)


def test_fitting_representation_builds_the_loader(dataset, capsys):
    from frlw_evd_amd import exp
    from frlw_evd_amd.recording_dataset import RecordingLoader
    raw, lab = dataset
    settings = types.SimpleNamespace(event_volume_bins=4, dataset_name="gen1", img_size=[256, 320], input_img_size=[256, 320], raw_dir=raw,
                                     bbox_path=lab, data_path=None, representation="taf", batch_size=4, gpu_device=torch.device("cpu"),
                                     synthetic=False)
    e = exp.yoloxtafBFM(settings)
    e._disk_loaders(test_only=True)
    assert isinstance(e.val_loader, RecordingLoader) and e.val_loader.channels == 8
    assert (e.nr_val_epochs, e.ori_width, e.ori_height, e.object_classes) == (3, 304, 240, ["Car", "Pedestrian"])
    assert "test_loader_len: 3" in capsys.readouterr().out
    settings.event_volume_bins = 5
    with pytest.raises(SystemExit, match="--event_volume_bins 8"):
        exp.yoloxtafBFM(settings)._disk_loaders(test_only=True)
    with pytest.raises(ValueError):   # training reads files
        exp.yoloxtafBFM(settings)._disk_loaders()


@pytest.mark.parametrize("shapes", restated.SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_restated_hand_off_equals_the_oracle_resize(shapes):
    from oracle import oracle as orc
    (h, w), (H, W) = shapes
    rng = np.random.default_rng(h * w + H)
    for Cn in (2, 10):
        srcs = [rng.integers(0, 256, (Cn + 1) * h * w + 3, dtype=np.uint8)[3 - b:][:Cn * h * w] for b in range(3)]   # any byte offset
        got = restated.hand_off(srcs, Cn, (h, w), (H, W))
        want = np.stack([orc.resize_nearest(s.reshape(Cn, h, w).astype(np.float32), (H, W)) / np.float32(255) for s in srcs])
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()


def test_library_exports_the_hand_off():
    from frlw_evd_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "frlw_volume_hand_off_u8") and "frlw_volume_hand_off_u8" in _lib.SYMBOLS
    assert "frlw_volume_hand_off_u8(" in open(os.path.join(ROOT, "include", "frlw_evd.h")).read()
    # argument checks answer before anything is launched: no GPU needed
    assert lib.frlw_volume_hand_off_u8(None, 1, 2, 8, 8, 8, 8, None, None) == _lib.FRLW_ERR_ARG


@pytest.mark.parametrize("key", list(red.ENTRY_CASES))
def test_cpu_forward_finds_boxes(dataset, key):
    """No GPU code here: the oracle's volumes of the planned labels, nearest resize and ``/255`` in numpy, the torch CPU forward with
    decode and NMS of the case's recipe weights, the evaluator's host arithmetic -> between 1 and 200 boxes on at least half of
    the frames the evaluator keeps (ground truth behind 0.5 s)."""
    from frlw_evd_amd.evaluator import evaluator
    raw, lab = dataset
    case = red.ENTRY_CASES[key]
    inputs = red.oracle_inputs(raw, lab, case)
    assert [(n, t) for n, t, _ in inputs] == red.planned_samples(raw, lab, "taf" if case["representation"] == "taf" else "ev")
    net = red.build_net(case)
    with torch.no_grad():
        dets = net.detect(torch.from_numpy(np.stack([v for _, _, v in inputs]))[..., None])
    ev = evaluator(None, 4, 10000, 304, 240, 320, 256, "gen1")
    kept = [(t, red.real_rows(ev.filter_boxes(ev.transform_dt(d, t)))) for d, (_, t, _) in zip(dets, inputs) if t > 500_000]
    print(key, kept)
    assert len(kept) == 7 and sum(1 <= c <= 200 for _, c in kept) >= (len(kept) + 1) // 2, kept

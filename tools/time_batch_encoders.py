#!/usr/bin/env python3
"""Timings of the batched Event Count Image / Surface of Active Events encoders and of the per-file label calls against the
single calls they replace, same box, same run, one JSON line each:

  eci     64 windows x 100 000 events at 304x240: one encode_eci_batch against 64 encode_eci_dat calls
  sae     64 streams x 1 000 000 events, 3 lamdas:  one encode_sae_batch against 64 encode_sae_dat calls
  chain   64 chained steps x 100 000 events, 3 lamdas: one encode_sae_chain against 64 encode_sae_dat calls fed their memory
  ranges  64 overlapping windows x 100 000 events (each starts 25 000 records after the one before), 5 bins: one
          encode_ev_ranges against 64 encode_ev_dat calls
  taf_chain  one stream of 64 windows x about 20 000 events, K = 8: one encode_taf_chain that hands out the volume after every
          window (64 snapshots) and after every fifth (12 snapshots) against the same volumes from per-step encode_taf_dat calls
          with the state carried
  taf_generate  wall time of generate.generate_taf on the fabricated dataset of tests/harness_data.py; with
          ``--parent_generate <generate.py of the parent commit>`` that file's generate_taf is timed on the same dataset in the
          same process and the two output trees are compared byte for byte

Device events around `n` back-to-back repetitions, `--runs` (>= 5) such regions after a warm-up; the value is the median, the
spread min .. max.  Both sides are timed unchecked (``check=False``: no host synchronisation, the device's best case for the
single calls) and checked (their default).  GB/s = 8 bytes per record plus the planes written (and the memory read), over the
batched call's time.  Each side runs in a child process of its own under a time limit; the parent never opens the GPU and
starts nothing more after a child that did not end normally.

``python tools/time_batch_encoders.py [--runs 7] [--sides chain,ranges] [--out profiles/label_batches_time.txt]``
``python tools/time_batch_encoders.py --sides taf_chain,taf_generate [--parent_generate FILE] --out profiles/taf_chain_time.txt``
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, B = 240, 304, 64
LAMDAS = [0.00001, 0.0000025, 0.000001]
LIMIT_S = {"eci": 240, "sae": 420, "chain": 240, "ranges": 240, "taf_chain": 240, "taf_generate": 240}
PARENT_GENERATE = None   # --parent_generate


def regions(fn, runs, n, warm=2):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n)
    return out


def report(name, ms, **extra):
    import numpy as np
    row = {"what": name, "ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
           "runs": len(ms)}
    row.update(extra)
    print(json.dumps(row), flush=True)
    return float(np.median(ms))


def streams(n_distinct, n, seed, t_offset=0):
    """B streams of n events back to back (n_distinct different ones, repeated) as one (B * n, 8) uint8 device tensor."""
    import numpy as np
    import torch
    from frlw_evd_amd import synth
    parts = [synth.to_dat8(synth.synth_events(seed + k, n, W, H, 1_000_000, hotspot=bool(k & 1), t_offset=t_offset)) for k in range(n_distinct)]
    rec = np.concatenate([parts[s % n_distinct] for s in range(B)])
    return torch.from_numpy(rec.view(np.uint8).reshape(-1, 8).copy()).cuda()


def side_eci(runs):
    import torch
    from frlw_evd_amd import event_representation as er
    n = 100_000
    dat = streams(16, n, 100)
    ranges = [(s * n, (s + 1) * n) for s in range(B)]
    parts = [dat[lo:hi] for lo, hi in ranges]
    f32, _ = er.encode_eci_batch(dat, ranges, (H, W))
    assert all(torch.equal(f32[s], er.encode_eci_dat(parts[s], (H, W))[0]) for s in range(B))
    nbytes = B * n * 8 + B * 2 * H * W * 4
    res = {}
    for check in (False, True):
        tag = "checked" if check else "unchecked"
        res["b", check] = report(f"eci batch: 1 call, {B} windows x {n} events, {tag}",
                                 regions(lambda: er.encode_eci_batch(dat, ranges, (H, W), check=check), runs, 10))
        res["s", check] = report(f"eci single: {B} calls x {n} events, {tag}",
                                 regions(lambda: [er.encode_eci_dat(p, (H, W), check=check) for p in parts], runs, 3))
        er.raise_deferred()
    print(json.dumps({"what": "eci: batched / 64 single calls", "ratio_unchecked": round(res["b", False] / res["s", False], 4),
                      "ratio_checked": round(res["b", True] / res["s", True], 4), "bytes": nbytes,
                      "batched_GB_per_s": round(nbytes / res["b", False] / 1e6, 1),
                      "us_per_window_batched": round(res["b", False] * 1e3 / B, 2), "us_per_single_call": round(res["s", False] * 1e3 / B, 2)}),
          flush=True)


def side_sae(runs):
    import torch
    from frlw_evd_amd import event_representation as er
    n = 1_000_000
    now, win = 11_000_500, 800_000
    dat = streams(8, n, 200, t_offset=10_000_000)
    offs = [s * n for s in range(B + 1)]
    parts = [dat[offs[s]:offs[s + 1]] for s in range(B)]
    mem = torch.full((B, 2, H, W), 9_000_000.0, device="cuda")
    f32, _, m = er.encode_sae_batch(dat, offs, (H, W), LAMDAS, mem, now, win)
    for s in (0, 1, B - 1):
        f1, _, m1 = er.encode_sae_dat(parts[s], (H, W), LAMDAS, mem[s], now, win)
        assert torch.equal(f32[s], f1) and torch.equal(m[s], m1)
    nbytes = B * n * 8 + B * 2 * H * W * 4 * (2 + len(LAMDAS))   # records, memory in and out, the f32 decays
    res = {}
    for check in (False, True):
        tag = "checked" if check else "unchecked"
        res["b", check] = report(f"sae batch: 1 call, {B} streams x {n} events, {tag}",
                                 regions(lambda: er.encode_sae_batch(dat, offs, (H, W), LAMDAS, mem, now, win, check=check), runs, 3))
        res["s", check] = report(f"sae single: {B} calls x {n} events, {tag}",
                                 regions(lambda: [er.encode_sae_dat(parts[s], (H, W), LAMDAS, mem[s], now, win, check=check)
                                                  for s in range(B)], runs, 2))
        er.raise_deferred()
    print(json.dumps({"what": "sae: batched / 64 single calls", "ratio_unchecked": round(res["b", False] / res["s", False], 4),
                      "ratio_checked": round(res["b", True] / res["s", True], 4), "bytes": nbytes,
                      "batched_GB_per_s": round(nbytes / res["b", False] / 1e6, 1),
                      "us_per_stream_batched": round(res["b", False] * 1e3 / B, 2), "us_per_single_call": round(res["s", False] * 1e3 / B, 2)}),
          flush=True)


def side_chain(runs):
    import torch
    from frlw_evd_amd import event_representation as er
    n = 100_000
    win = 800_000
    dat = streams(16, n, 300, t_offset=10_000_000)
    steps = [(s * n, (s + 1) * n, 11_000_500 + 1_000 * s, win, True) for s in range(B)]   # every step emits its volume
    mem = torch.full((2, H, W), 9_000_000.0, device="cuda")

    def single(check):
        m, out = mem, None
        for lo, hi, now, w, _ in steps:
            out, _, m = er.encode_sae_dat(dat[lo:hi], (H, W), LAMDAS, m, now, w, check=check)
        return out, m

    f32, _, m = er.encode_sae_chain(dat, steps, (H, W), LAMDAS, mem)
    f1, m1 = single(True)
    assert torch.equal(f32[B - 1], f1) and torch.equal(m, m1)
    nbytes = B * n * 8 + 2 * H * W * 4 * (2 + B * len(LAMDAS)) + B * 2 * H * W * 8   # records, memory, the f32 decays, the key planes
    res = {}
    for check in (False, True):
        tag = "checked" if check else "unchecked"
        res["b", check] = report(f"sae chain: 1 call, {B} steps x {n} events, {tag}",
                                 regions(lambda: er.encode_sae_chain(dat, steps, (H, W), LAMDAS, mem, check=check), runs, 10))
        res["s", check] = report(f"sae single: {B} chained calls x {n} events, {tag}", regions(lambda: single(check), runs, 3))
        er.raise_deferred()
    print(json.dumps({"what": "sae chain: one call / 64 single calls", "ratio_unchecked": round(res["b", False] / res["s", False], 4),
                      "ratio_checked": round(res["b", True] / res["s", True], 4), "bytes": nbytes,
                      "chain_GB_per_s": round(nbytes / res["b", False] / 1e6, 1),
                      "us_per_step_chained": round(res["b", False] * 1e3 / B, 2), "us_per_single_call": round(res["s", False] * 1e3 / B, 2)}),
          flush=True)


def side_ranges(runs):
    import numpy as np
    import torch
    from frlw_evd_amd import event_representation as er, synth
    n, hop, win, bins = 100_000, 25_000, 250_000, 5
    total = (B - 1) * hop + n
    rec = synth.to_dat8(synth.synth_events(400, total, W, H, win * total // n, hotspot=True, t_offset=win + 1))   # a window's 100 000 records span about `win`
    dat = torch.from_numpy(rec.view(np.uint8).reshape(-1, 8).copy()).cuda()
    ranges = [(s * hop, s * hop + n) for s in range(B)]
    t_end = [int(rec["t"][hi - 1]) for _, hi in ranges]
    parts = [dat[lo:hi] for lo, hi in ranges]
    f32, _ = er.encode_ev_ranges(dat, ranges, (H, W), t_end, win, bins)
    for s in (0, 1, B - 1):
        assert torch.equal(f32[s], er.encode_ev_dat(parts[s], (H, W), t_end[s], win, bins)[0])
    nbytes = 3 * B * n * 8 + B * 2 * bins * H * W * 4   # records read, copied and read again, the f32 volumes
    res = {}
    for check in (False, True):
        tag = "checked" if check else "unchecked"
        res["b", check] = report(f"ev ranges: 1 call, {B} windows x {n} events, {tag}",
                                 regions(lambda: er.encode_ev_ranges(dat, ranges, (H, W), t_end, win, bins, check=check), runs, 10))
        res["s", check] = report(f"ev single: {B} calls x {n} events, {tag}",
                                 regions(lambda: [er.encode_ev_dat(parts[s], (H, W), t_end[s], win, bins, check=check) for s in range(B)], runs, 3))
        er.raise_deferred()
    print(json.dumps({"what": "ev ranges: one call / 64 single calls", "ratio_unchecked": round(res["b", False] / res["s", False], 4),
                      "ratio_checked": round(res["b", True] / res["s", True], 4), "bytes": nbytes,
                      "ranges_GB_per_s": round(nbytes / res["b", False] / 1e6, 1),
                      "us_per_window_ranged": round(res["b", False] * 1e3 / B, 2), "us_per_single_call": round(res["s", False] * 1e3 / B, 2)}),
          flush=True)


def side_taf_chain(runs):
    import numpy as np
    import torch
    from frlw_evd_amd import event_representation as er, synth
    K, win, n_win, per = 8, 10_000, 64, 20_000
    rec = synth.to_dat8(synth.synth_events(500, n_win * per, W, H, n_win * win, hotspot=True))
    dat = torch.from_numpy(rec.view(np.uint8).reshape(-1, 8).copy()).cuda()
    fresh = torch.full((H, W, 2, K), -6000.0, device="cuda")
    state = fresh.clone()
    for name, bins in (("every window: 64 snapshots", [1] * 64), ("every fifth window: 12 snapshots", [5] * 12)):
        S = len(bins)
        ends = np.cumsum(bins) * win
        cuts = [0] + [int(c) for c in np.searchsorted(rec["t"], ends[:-1], side="left")] + [int(np.searchsorted(rec["t"], ends[-1], side="left"))]
        parts = [dat[cuts[s]:cuts[s + 1]] for s in range(S)]
        whole = dat[:cuts[-1]]

        def chain(check):
            state.copy_(fresh)
            return er.encode_taf_chain(whole, (H, W), state, 0, win, bins, K, check=check)

        def steps(check):
            state.copy_(fresh)
            return [er.encode_taf_dat(parts[s], (H, W), state, int(ends[s]) - bins[s] * win, win, bins[s], K, check=check, fast=False)[0]
                    for s in range(S)]

        a = chain(True)
        sa = state.clone()
        b = steps(True)
        assert torch.equal(a, torch.stack(b)) and torch.equal(sa, state)
        nbytes = cuts[-1] * 8 + 2 * H * W * 2 * K * 4 + S * 2 * K * H * W   # records, the state in and out, the uint8 volumes
        res = {}
        for check in (False, True):
            tag = "checked" if check else "unchecked"
            res["b", check] = report(f"taf chain, {name}: 1 call, {cuts[-1]} events, {tag}", regions(lambda: chain(check), runs, 10))
            res["s", check] = report(f"taf per step, {name}: {S} encode_taf_dat calls, {tag}", regions(lambda: steps(check), runs, 3))
            er.raise_deferred()
        print(json.dumps({"what": f"taf chain, {name}: one call / {S} per-step calls", "ratio_unchecked": round(res["b", False] / res["s", False], 4),
                          "ratio_checked": round(res["b", True] / res["s", True], 4), "bytes": nbytes,
                          "chain_GB_per_s": round(nbytes / res["b", False] / 1e6, 1),
                          "us_per_snapshot_chained": round(res["b", False] * 1e3 / S, 2), "us_per_step_call": round(res["s", False] * 1e3 / S, 2)}),
              flush=True)


def side_taf_generate(runs):
    import filecmp
    import importlib.util
    import tempfile
    import time

    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import harness_data
    from frlw_evd_amd import generate
    arms = [("this tree", generate)]
    if PARENT_GENERATE:
        spec = importlib.util.spec_from_file_location("frlw_evd_amd.generate_parent", PARENT_GENERATE)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
        arms.append(("parent", parent))
    with tempfile.TemporaryDirectory() as root:
        raw, lab = harness_data.build(root)
        trees = []
        for name, mod in arms:
            target = os.path.join(root, "out_" + name.replace(" ", "_"))
            secs, files = [], 0
            for r in range(runs + 1):   # the first run is the warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                files = mod.generate_taf(raw, lab, target, "gen1")
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - t0)
            secs = secs[1:]
            print(json.dumps({"what": f"generate_taf on harness_data, {name}", "files": files, "s_median": round(float(np.median(secs)), 4),
                              "s_min": round(min(secs), 4), "s_max": round(max(secs), 4), "runs": len(secs)}), flush=True)
            trees.append(target)
        if len(trees) == 2:
            def same(a, b):
                c = filecmp.dircmp(a, b)
                if c.left_only or c.right_only or c.funny_files:
                    return False
                _, mismatch, errors = filecmp.cmpfiles(a, b, c.common_files, shallow=False)
                return not mismatch and not errors and all(same(os.path.join(a, d), os.path.join(b, d)) for d in c.common_dirs)
            print(json.dumps({"what": "generate_taf: output trees of the two arms byte-identical", "identical": same(*trees)}), flush=True)


SIDES = {"eci": side_eci, "sae": side_sae, "chain": side_chain, "ranges": side_ranges, "taf_chain": side_taf_chain,
         "taf_generate": side_taf_generate}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--only", choices=tuple(SIDES))
    ap.add_argument("--sides", default=",".join(SIDES), help="comma-separated subset of " + ", ".join(SIDES))
    ap.add_argument("--out")
    ap.add_argument("--parent_generate", help="taf_generate: the parent commit's frlw_evd_amd/generate.py, timed beside this tree's")
    a = ap.parse_args()
    assert a.runs >= 5
    global PARENT_GENERATE
    PARENT_GENERATE = a.parent_generate
    if a.only:
        import torch
        from frlw_evd_amd import _lib
        print(json.dumps({"device": torch.cuda.get_device_name(0), "library": _lib.load().frlw_version().decode(), "side": a.only}), flush=True)
        SIDES[a.only](a.runs)
        return 0
    text = ""
    for side in a.sides.split(","):
        if side not in SIDES:
            ap.error(f"unknown side {side}")
        try:
            extra = ["--parent_generate", a.parent_generate] if a.parent_generate else []
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", side, "--runs", str(a.runs)] + extra, capture_output=True,
                               text=True, timeout=LIMIT_S[side])
        except subprocess.TimeoutExpired:
            print(f"{side}: no result inside {LIMIT_S[side]} s; nothing more is started", file=sys.stderr)
            return 1
        sys.stdout.write(p.stdout)
        text += p.stdout
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            print(f"{side}: exit status {p.returncode}; nothing more is started", file=sys.stderr)
            return 1
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Copy what tools/xcd_ab.sh left in its output directory (argv[1], default build/xcd_ab/) into profiles/ (prefix xcd_) and rebuild profiles/traffic_*.json from the
child's PMC summaries, as tools/collect_r06.py does: FETCH_SIZE (KiB) x 1024 x 2 (gfx950 reports half of a coalesced read),
WRITE_SIZE (KiB) x 1024, tagged with the hash of the kernel sources.  Every traffic file also carries the parent's figures from
the same run (`parent_per_kernel`, `parent_hbm_bytes_per_encode`): the A/B of the consumers' XCD mapping."""
import hashlib, json, os, re, shutil, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "build", "xcd_ab")
P = os.path.join(ROOT, "profiles")


def sha():
    h = hashlib.sha256()
    for name in ("taf_fast.hip", "partition.hip", "encoders.hip", "frlw_common.h"):
        h.update(open(os.path.join(ROOT, "frlw-evd_amd", "csrc", name), "rb").read())
    return h.hexdigest()[:16]


def per_kernel(path):
    per, cur = {}, None
    for line in open(path):
        if not line.startswith(" "):
            cur = line.strip(); continue
        m = re.match(r"\s+(\S+)\s+(\d+)", line)
        if m and cur:
            per.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    tot, out = 0, {}
    for k, v in per.items():
        if "FETCH_SIZE" in v and k.startswith("kf_") and "selftest" not in k:  # (the self-test runs once per process, not per encode)
            f, w = v["FETCH_SIZE"] * 1024 * 2, v.get("WRITE_SIZE", 0) * 1024
            o = out.setdefault(k.split("<")[0], {"fetch_bytes_corrected": 0, "write_bytes": 0})
            o["fetch_bytes_corrected"] += f; o["write_bytes"] += w
            tot += f + w
    return tot, out


def traffic(cfg, tag, alg, how):
    tot, out = per_kernel(os.path.join(O, f"child_{cfg}_pmc_summary.txt"))
    ptot, pout = per_kernel(os.path.join(O, f"parent_{cfg}_pmc_summary.txt"))
    json.dump({"workload": tag, "hbm_bytes_per_encode": tot, "algorithmic_bytes": alg, "ratio": round(tot / alg, 3),
               "kernel_source_sha": sha(),
               "method": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE in separate passes over `" + how + "` (tools/xcd_ab.sh: the same "
                         "kernels on a stream of the same shape), per-dispatch averages, KiB x 1024, FETCH_SIZE doubled per "
                         "MI355X_MICROARCH.md (gfx950 reports half of a coalesced read); parent_*: the parent commit's library, same box, same run",
               "per_kernel": out, "parent_hbm_bytes_per_encode": ptot, "parent_ratio": round(ptot / alg, 3), "parent_per_kernel": pout,
               "source": f"profiles/xcd_child_{cfg}_pmc_summary.txt"},
              open(os.path.join(P, f"traffic_{tag}.json"), "w"), indent=1)
    print(tag, "traffic MB", round(ptot / 1e6, 1), "->", round(tot / 1e6, 1), "ratio", round(ptot / alg, 3), "->", round(tot / alg, 3))


def bench_ab():
    """bench_ab.txt: roofline.device_ms of the alternating bench runs, per arm, in run order."""
    import glob, statistics as st
    L = ["bench.py A/B of the consumers' XCD mapping: parent commit's library against this one, ONE box, arms alternating (parent, child, parent, ...).",
         "roofline.device_ms per run, in run order.\n"]
    for tag, cmd in (("head", "python bench.py --gpus 1   (50 steps, every leg)"),
                     ("gen1", "python bench.py --gpus 1 --workload taf_gen1 --no-detector --no-train --no-also --no-cpu-baseline   (50 steps)")):
        L.append(cmd)
        for arm in ("parent", "child"):
            v = [json.load(open(f))["roofline"]["device_ms"] for f in sorted(glob.glob(os.path.join(O, f"ab_{tag}_{arm}_*.json")))]
            L.append(f"  {arm:6s} {v}  median {st.median(v):.4f}  min {min(v):.4f}  max {max(v):.4f}")
        L.append("")
    L.append("python bench.py --gpus 1 --full --no-detector --no-train   (one run per arm)")
    keys = ["device_ms", "gen1_taf_x64_ms", "gen1_ev_x64_ms", "taf_mpx_hotspot_ms", "gen1_taf_single_eager_ms", "gen1_taf_single_graph_ms",
            "gen1_ev_single_eager_ms", "gen1_ev_single_default_call_ms"]
    for arm in ("parent", "child"):
        r = json.load(open(os.path.join(O, f"ab_full_{arm}_1.json")))["roofline"]
        L.append(f"  {arm:6s} " + "  ".join(f"{k} {r.get(k)}" for k in keys))
    L.append("\nbench.py --dump-outputs of the two arms: taf_u8.npy and taf_state_sample.npy cmp-equal (tools/xcd_ab.sh stops otherwise).")
    open(os.path.join(O, "bench_ab.txt"), "w").write("\n".join(L) + "\n")


bench_ab()
for f in sorted(os.listdir(O)):
    if f.endswith("_pmc_summary.txt") or f.endswith("_kernel_stats.csv") or f in ("lab.txt", "lab_nofadd.txt", "bench_ab.txt"):
        text = open(os.path.join(O, f)).read()
        if f.startswith("lab"):  # the harness prints the libraries' full paths: keep them relative to the repository
            text = "".join(l for l in re.sub(r"(/[\w.+-]+)+/(build/libfrlw_base\.so|frlw-evd_amd/csrc/libfrlw_evd\.so)", r"\2", text).splitlines(True)
                           if not l.startswith("rc="))
        open(os.path.join(P, "xcd_" + f), "w").write(text)
taf = lambda n, H, W, K=8: 8 * n + 2 * 4 * 2 * K * H * W + 2 * K * H * W
ev = lambda n, H, W, b=5: 8 * n + 4 * 2 * b * H * W
lab = lambda c: f"build/enc_lab <lib> --cfg {c}"
traffic("mpx", "taf_mpx", taf(10_000_000, 720, 1280), lab("mpx"))
traffic("mpx_hot", "taf_mpx_hotspot", taf(10_000_000, 720, 1280), lab("mpx_hot"))
traffic("gen1", "taf_gen1", taf(1_000_000, 240, 304), lab("gen1"))
traffic("gen1x64", "taf_gen1_x64", 64 * taf(1_000_000, 240, 304), lab("gen1x64"))   # (the lab's sequences are ragged: a few % fewer events)
traffic("evb1", "ev_gen1", ev(1_000_000, 240, 304), lab("evb1"))
traffic("evb64", "ev_gen1_x64", 64 * ev(1_000_000, 240, 304), lab("evb64"))
traffic("sae", "sae_gen1", 8 * 1_000_000 + 2 * 4 * 2 * 240 * 304 + 4 * 6 * 240 * 304, "python tools/run_small_encoders.py sae")
traffic("eci", "eci_gen1", 8 * 100_000 + 4 * 2 * 240 * 304, "python tools/run_small_encoders.py eci")

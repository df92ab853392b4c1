"""Sampling decode against greedy ensemble decode, timed in graph mode at configs[3]'s decode shape (B 16, max_length 80, the cfg2
model of bench.py; untrained, so nearly every row runs all 80 steps).

(a) Ensemble([m]).beamsearch_decode(beam_size=1) in this tree and, with --other-tree DIR, in another checkout of the project (the
    parent commit, built): per step the member's decoder step and head, then vag_ens_argmax;
(b) m.sample_decode(n_samples=1) with top_k 0 and 10 in this tree: per step the member's decoder step and head, then
    vag_sample_step_dev in the arg-max's place.  Not the same member launches: the ensemble's captured greedy steps are the hoisted
    ones where the shape allows, the sampler's are the plain ones in both modes, so the difference between (a) and
    (b) is the sampler against the arg-max PLUS plain against hoisted steps;
(c) the step launches alone on synthetic rows (N 16 and 192, V 9391): vag_ens_argmax, vag_sample_step top_k 0 / 10 / 64.

The measurements alternate, one fresh process each, so that all see the same box in the same session.  Every figure: host clock
around `reps` calls closed by a device synchronise, after a warm-up; `windows` such windows per process, all of them reported.
Every measuring process runs under a time limit of its own; after one that fails or runs out of time nothing more is started.

Usage (GPU box):  python tools/exp_sample.py [--other-tree DIR] [--rounds 3] [--windows 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 300               # one measuring process: import, build the model, capture, warm up, time
B, ML, V3 = 16, 80, 9391


def windows_of(fn, reps, windows):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps)
    return out


def summary(xs, scale):
    return {"median": statistics.median(xs) * scale, "min": min(xs) * scale, "max": max(xs) * scale,
            "windows": [x * scale for x in xs]}


def worker(mode, tree, windows):
    """One measurement in the checkout `tree` (this process imports that tree's package and bench.py)."""
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "vag-nmt_amd"))
    import torch
    res = {"mode": mode, "tree": tree, "device": torch.cuda.get_device_name(0)}
    dev = torch.device("cuda:0")
    if mode == "launch":
        import ctypes as C
        from vagnmt_hip._lib import call, ptr, stream
        I64 = torch.int64
        for N in (16, 192):
            ldl = (V3 + 3) // 4 * 4
            x = torch.log_softmax(torch.randn(N, ldl, device=dev) * 3, 1)
            pp, ld = (C.c_void_p * 1)(x.data_ptr()), (C.c_int64 * 1)(ldl)
            out = torch.empty(N, dtype=I64, device=dev)
            toks = torch.full((2, N), 5, dtype=I64, device=dev)
            lps = torch.zeros(2, N, device=dev)
            alive = torch.zeros(3, dtype=torch.int32, device=dev)
            rng = torch.tensor([1, 0], dtype=I64, device=dev)
            xs = windows_of(lambda: call("vag_ens_argmax", pp, ld, 1, N, V3, ptr(out, I64), stream()), 500, windows)
            res["argmax_N%d_us" % N] = summary(xs, 1e6)
            for k in (0, 10, 64):
                xs = windows_of(lambda: call("vag_sample_step", pp, ld, 1, ptr(toks, I64), ptr(lps), 1, 2, None, None, None,
                                             ptr(out, I64), N, 1, V3, 1.0, k, ptr(rng, I64), ptr(alive, torch.int32), stream()),
                                500, windows)
                res["sample_top%d_N%d_us" % (k, N)] = summary(xs, 1e6)
        res["row_bytes"] = V3 * 4
        print("RESULT " + json.dumps(res))
        return
    import bench
    from vagnmt_hip.ensemble import Ensemble
    c = dict(bench.CFG2)
    c["B"] = B
    m = bench.build_model(c, dev).eval()
    src, lens, _, im = bench.make_batch(c, 0, dev, ragged=True)
    if mode == "greedy":
        ens = Ensemble([m])
        fn = lambda: ens.beamsearch_decode(src, lens, im, 1, ML)
        steps_of = lambda: int(ens.last_decode_steps)
    else:
        from vagnmt_hip.sampling import Generator
        gen, k = Generator(1), int(mode[6:])
        fn = lambda: m.sample_decode(src, lens, im, n_samples=1, max_length=ML, temperature=1.0, top_k=k, generator=gen)
        steps_of = lambda: int(m.last_decode_steps)
    xs = windows_of(fn, 10, windows)
    steps = steps_of()
    res.update(steps=steps, us_per_step=summary(xs, 1e6 / steps), ms_per_batch=summary(xs, 1e3))
    print("RESULT " + json.dumps(res))


def run_child(mode, tree, windows):
    """A fresh process per measurement, under its own time limit; None after a failure (the caller then stops)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--tree", tree, "--windows", str(windows)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        print("%s in %s: no result within %d s -- stopping" % (mode, tree, STEP_LIMIT_S))
        return None
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        print("%s in %s: exit status %d -- stopping\n%s" % (mode, tree, r.returncode, r.stderr[-2000:]))
        return None
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-tree", default=None, help="another built checkout (the parent commit) for the greedy ensemble decode")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, choices=["greedy", "sample0", "sample10", "launch"])
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, os.path.abspath(a.tree), a.windows)
    runs = [("greedy_this", "greedy", ROOT), ("sample_top0", "sample0", ROOT), ("sample_top10", "sample10", ROOT)]
    if a.other_tree:
        runs.insert(0, ("greedy_other", "greedy", os.path.abspath(a.other_tree)))
    res = {"shape": dict(B=B, n_samples=1, max_length=ML), "decode": {name: [] for name, _, _ in runs}, "launch": None}
    ok = True
    for r in range(a.rounds):
        for name, mode, tree in (runs if r % 2 == 0 else runs[::-1]):          # alternate, and alternate who goes first
            got = run_child(mode, tree, a.windows) if ok else None
            ok = ok and got is not None
            if got:
                res["decode"][name].append(got)
                print("round %d %-13s %.1f us per decode step over %d steps (windows %.1f .. %.1f)" % (
                    r, name, got["us_per_step"]["median"], got["steps"], got["us_per_step"]["min"], got["us_per_step"]["max"]))
    if ok:
        res["launch"] = run_child("launch", ROOT, a.windows)
        ok = res["launch"] is not None
    for name, _, _ in runs:
        meds = [g["us_per_step"]["median"] for g in res["decode"][name]]
        allw = [w for g in res["decode"][name] for w in g["us_per_step"]["windows"]]
        if meds:
            res[name + "_us_per_step"] = {"median_of_medians": statistics.median(meds), "process_medians": meds,
                                          "min_window": min(allw), "max_window": max(allw)}
    if res["launch"]:
        for key, v in sorted(res["launch"].items()):
            if key.endswith("_us"):
                print("%-22s %.2f us (windows %.2f .. %.2f)" % (key, v["median"], v["min"], v["max"]))
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""Nucleus (top-p) sampling against plain sampling, timed in graph mode at configs[3]'s decode shape (B 16, max_length 80, the cfg2
model of bench.py; untrained, so nearly every row runs all 80 steps and its distribution is nearly flat: a nucleus of top_p 0.9
holds most of the 9391 words, the threshold search's full cost with no small-set shortcut).

(a) m.sample_decode(n_samples=1, top_k=0) with top_p 1.0 (the plain decode: vag_sample_step_dev per step) and with top_p 0.9
    (vag_sample_step_p_dev in its place; the member launches are the same), both in this tree;
(b) the step launches alone on synthetic rows (N 16 and 192, V 9391, log_softmax(3 normal)): vag_sample_step top_k 0 / 64
    against vag_sample_step_p at top_p 0.9 (top_k 0 and 64), 0.5 (top_k 0) and 1.0 (top_k 0: the whole pool, no search).

The measurements alternate, one fresh process each, so that all see the same box in the same session.  Every figure: host clock
around `reps` calls closed by a device synchronise, after a warm-up; `windows` such windows per process, all of them reported.
Every measuring process runs under a time limit of its own; after one that fails or runs out of time nothing more is started.

Usage (GPU box):  python tools/exp_nucleus.py [--rounds 3] [--windows 5] [--out FILE]"""
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


def worker(mode, windows):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "vag-nmt_amd"))
    import torch
    res = {"mode": mode, "device": torch.cuda.get_device_name(0)}
    dev = torch.device("cuda:0")
    if mode == "launch":
        import ctypes as C
        from vagnmt_hip._lib import call, ptr, stream
        I64, I32 = torch.int64, torch.int32
        for N in (16, 192):
            ldl = (V3 + 3) // 4 * 4
            x = torch.log_softmax(torch.randn(N, ldl, device=dev) * 3, 1)
            pp, ld = (C.c_void_p * 1)(x.data_ptr()), (C.c_int64 * 1)(ldl)
            out = torch.empty(N, dtype=I64, device=dev)
            toks = torch.full((2, N), 5, dtype=I64, device=dev)
            lps = torch.zeros(2, N, device=dev)
            sizes = torch.zeros(2, N, dtype=I32, device=dev)
            alive = torch.zeros(3, dtype=I32, device=dev)
            rng = torch.tensor([1, 0], dtype=I64, device=dev)
            head = lambda k: (pp, ld, 1, ptr(toks, I64), ptr(lps), 1, 2, None, None, None, ptr(out, I64), N, 1, V3, 1.0, k,
                              ptr(rng, I64), ptr(alive, I32))
            for k in (0, 64):
                xs = windows_of(lambda: call("vag_sample_step", *head(k), stream()), 500, windows)
                res["plain_top%d_N%d_us" % (k, N)] = summary(xs, 1e6)
            for k, p in ((0, 0.9), (64, 0.9), (0, 0.5), (0, 1.0)):
                xs = windows_of(lambda: call("vag_sample_step_p", *head(k), p, ptr(sizes, I32), stream()), 500, windows)
                torch.cuda.synchronize()
                res["nucleus_top%d_p%.1f_N%d_us" % (k, p, N)] = summary(xs, 1e6)
                res["nucleus_top%d_p%.1f_N%d_sizes" % (k, p, N)] = [int(sizes[1].min()), int(sizes[1].max())]
        res["row_bytes"] = V3 * 4
        print("RESULT " + json.dumps(res))
        return
    import bench
    from vagnmt_hip.sampling import Generator
    c = dict(bench.CFG2)
    c["B"] = B
    m = bench.build_model(c, dev).eval()
    src, lens, _, im = bench.make_batch(c, 0, dev, ragged=True)
    gen, p = Generator(1), float(mode[1:])
    fn = lambda: m.sample_decode(src, lens, im, n_samples=1, max_length=ML, temperature=1.0, top_k=0, top_p=p, generator=gen)
    xs = windows_of(fn, 10, windows)
    steps = int(m.last_decode_steps)
    _, sizes = m.sample_decode(src, lens, im, n_samples=1, max_length=ML, temperature=1.0, top_k=0, top_p=p, generator=gen,
                               return_sizes=True)
    live = sizes[sizes > 0]
    res.update(steps=steps, us_per_step=summary(xs, 1e6 / steps), ms_per_batch=summary(xs, 1e3),
               sizes=[int(live.min()), int(live.float().mean()), int(live.max())])
    print("RESULT " + json.dumps(res))


def run_child(mode, windows):
    """A fresh process per measurement, under its own time limit; None after a failure (the caller then stops)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--windows", str(windows)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        print("%s: no result within %d s -- stopping" % (mode, STEP_LIMIT_S))
        return None
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        print("%s: exit status %d -- stopping\n%s" % (mode, r.returncode, r.stderr[-2000:]))
        return None
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, choices=["p1.0", "p0.9", "launch"])
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.windows)
    runs = [("sample_top_p_1.0", "p1.0"), ("sample_top_p_0.9", "p0.9")]
    res = {"shape": dict(B=B, n_samples=1, max_length=ML, top_k=0), "decode": {name: [] for name, _ in runs}, "launch": None}
    ok = True
    for r in range(a.rounds):
        for name, mode in (runs if r % 2 == 0 else runs[::-1]):                 # alternate, and alternate who goes first
            got = run_child(mode, a.windows) if ok else None
            ok = ok and got is not None
            if got:
                res["decode"][name].append(got)
                print("round %d %-17s %.1f us per decode step over %d steps (windows %.1f .. %.1f), nucleus sizes min/mean/max %s" % (
                    r, name, got["us_per_step"]["median"], got["steps"], got["us_per_step"]["min"], got["us_per_step"]["max"],
                    got["sizes"]))
    if ok:
        res["launch"] = run_child("launch", a.windows)
        ok = res["launch"] is not None
    for name, _ in runs:
        meds = [g["us_per_step"]["median"] for g in res["decode"][name]]
        allw = [w for g in res["decode"][name] for w in g["us_per_step"]["windows"]]
        if meds:
            res[name + "_us_per_step"] = {"median_of_medians": statistics.median(meds), "process_medians": meds,
                                          "min_window": min(allw), "max_window": max(allw)}
            print("%-17s %.1f us per decode step (median of %d process medians; windows %.1f .. %.1f)" % (
                name, statistics.median(meds), len(meds), min(allw), max(allw)))
    if res["launch"]:
        for key, v in sorted(res["launch"].items()):
            if key.endswith("_us"):
                print("%-28s %.2f us (windows %.2f .. %.2f)%s" % (key, v["median"], v["min"], v["max"],
                                                                 "  sizes %s" % res["launch"].get(key[:-2] + "sizes", "")
                                                                 if key.startswith("nucleus") else ""))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""Microseconds per decode step of the searches and of the sampling decoder, a built checkout of the parent commit (PARENT_ROOT: bench.py, vag-nmt_amd with its
library) against this tree, alternating child processes inside one call.  Fails without a GPU.
Usage: python tools/exp_beam_refactor_speed.py PARENT_ROOT OUT.txt [--children 3] [--windows 2] [--reps 5]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, K, ML = 16, 12, 80
CASES = ["decode12", "nbest_logp", "diverse", "required", "stochastic", "penalised", "constrained", "sample"]


def worker(root, windows, reps):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "vag-nmt_amd"))
    import torch
    import bench
    from vagnmt_hip import search
    from vagnmt_hip.sampling import Generator
    assert os.path.abspath(search.__file__).startswith(os.path.abspath(root)), search.__file__
    c = dict(bench.CFG2)
    c["B"] = B
    dev = torch.device("cuda:0")
    m = bench.build_model(c, dev).eval()
    src, lens, _, im = bench.make_batch(c, 0, dev, ragged=True)
    V = c["V"]
    gen = Generator(1)
    req = [[[4 + (13 * b + 2 * i) % (V - 4), 4 + (13 * b + 2 * i + 1) % (V - 4)] for i in range(2)] for b in range(B)]

    def nbest_logp():
        m.decode_raw_logits = False
        m.beamsearch_nbest(src, lens, im, K, K, ML)
        m.decode_raw_logits = True

    fns = {"decode12": lambda: m.beamsearch_decode(src, lens, im, beam_size=K, max_length=ML),
           "nbest_logp": nbest_logp,
           "diverse": lambda: m.beamsearch_diverse(src, lens, im, beam_size=K, n_groups=3, diversity=0.5, max_length=ML),
           "required": lambda: m.beamsearch_required(src, lens, im, beam_size=K, n_best=1, max_length=ML, required=req),
           "stochastic": lambda: m.beamsearch_stochastic(src, lens, im, n_samples=K, max_length=ML, generator=gen),
           "penalised": lambda: m.beamsearch_penalised(src, lens, im, beam_size=K, n_best=K, max_length=ML, beta=0.2, stepwise=True),
           "constrained": lambda: m.beamsearch_constrained(src, lens, im, beam_size=K, n_best=1, max_length=ML, no_repeat_ngram=3),
           "sample": lambda: m.sample_decode(src, lens, im, n_samples=K, max_length=ML, generator=gen)}
    out = {}
    for graph in (True, False):
        m.decode_graph = graph
        steps = {}
        for name in CASES:                       # warm-up: captures, code objects
            for _ in range(2):
                fns[name]()
            steps[name] = int(m.last_decode_steps)
        torch.cuda.synchronize()
        for w in range(windows):
            for name in (CASES if w % 2 == 0 else CASES[::-1]):
                t0 = time.perf_counter()
                for _ in range(reps):
                    fns[name]()
                torch.cuda.synchronize()
                out.setdefault("%s/%s" % ("graph" if graph else "eager", name), []).append(
                    (time.perf_counter() - t0) / reps / steps[name] * 1e6)
        out["steps/%s" % ("graph" if graph else "eager")] = steps
    print("SPEED_CHILD " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("out")
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--windows", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    roots = {"parent": os.path.abspath(a.parent), "branch": ROOT}
    data = {"parent": {}, "branch": {}}
    steps = {}
    for i in range(a.children):
        for side in ("parent", "branch"):
            env = dict(os.environ, VAG_LIB=os.path.join(roots[side], "vag-nmt_amd", "lib", "libvagnmt.so"))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", roots[side], str(a.windows), str(a.reps)],
                               capture_output=True, text=True, timeout=300, env=env)
            if r.returncode != 0:
                print("child %s %d failed (%d): stopping\n%s\n%s" % (side, i, r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
                return r.returncode or 1
            d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("SPEED_CHILD ")][-1][len("SPEED_CHILD "):])
            for key, xs in d.items():
                if key.startswith("steps/"):
                    steps[side + "/" + key] = xs
                else:
                    data[side].setdefault(key, []).extend(xs)
            print("child %s %d done" % (side, i), flush=True)
    lines = ["us per decode step, B %d, beam %d, max_length %d (bench.py configs[3] decode shape); %d child processes per side, alternating "
             "parent / branch, %d windows of %d decodes each per child after a warm-up; every window ends in a device synchronise"
             % (B, K, ML, a.children, a.windows, a.reps), "steps run: %s" % json.dumps(steps)]
    ok = True
    for key in sorted(data["parent"]):
        p, b = data["parent"][key], data["branch"][key]
        mp, mb, spread = statistics.median(p), statistics.median(b), max(p) - min(p)
        good = mb - mp <= spread
        ok = ok and good
        lines.append("%-18s parent median %7.1f (windows %s)  branch median %7.1f (windows %s)  diff %+6.1f  parent spread %5.1f  %s"
                     % (key, mp, " ".join("%.1f" % x for x in p), mb, " ".join("%.1f" % x for x in b), mb - mp, spread,
                        "ok" if good else "EXCEEDS"))
    lines.append("condition (branch median - parent median <= parent spread) holds for every case: %s" % ok)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        sys.exit(main())

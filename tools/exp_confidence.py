"""Cost of word-level confidence at BASELINE configs[1] size (B=64, Ts=Tt=40, H=512, V=9391, ldl 9392), on one GPU, all in one
process:

  * the whole call: token_confidence against score_translations on the same inputs, a model (M = 1) and an Ensemble of M = 3 -- both
    run every member's teacher-forced pass; they differ in the one launch (vag_forced_score, one gather per position) or two
    (vag_token_conf, every member's logits read once) behind it;
  * the row kernel alone: vag_token_conf on prepared logits against its byte count M * Tt*B * V * 4 (the sentence kernel, one wave
    per sentence over 40 positions, rides in the same call; it is timed alone by running the call on an all-pad target, where
    every row workgroup leaves after its span scan), with every position in the span (targets without EOS or padding) and with
    the batch's own ragged targets;
  * the unchanged paths: score_translations and beamsearch_decode (beam 12) with this build and, with --parent-lib, with a library
    built from the parent commit, alternating over --rounds rounds.

Warm-up, then timed windows of back-to-back calls between two events; the median window is reported, with the windows' spread.

    git worktree add ../parent HEAD~1 && make -C ../parent/vag-nmt_amd/csrc -j8
    python tools/exp_confidence.py --parent-lib ../parent/vag-nmt_amd/lib/libvagnmt.so --out profiles/exp_confidence.txt"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vag-nmt_amd")]

import torch  # noqa: E402

from exp_label_smoothing import windows  # noqa: E402

NEW_SYMBOLS = ("vag_token_conf",)


def load_parent(path):
    """The parent's library as a second, independent CDLL with every prototype it can have."""
    from vagnmt_hip import _lib
    L = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.PROTOS.items():
        if name in NEW_SYMBOLS:
            continue
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    import bench
    from vagnmt_hip import _lib, confidence, scoring
    from vagnmt_hip._lib import ptr, stream
    from vagnmt_hip.ensemble import Ensemble
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def row(what, w):
        say("%-58s median %8.4f ms  spread %.4f ms  (windows %s)"
            % (what, statistics.median(w), max(w) - min(w), " ".join("%.4f" % x for x in w)))
        return statistics.median(w)
    c = bench.CFG2
    dev = torch.device("cuda", 0)
    say("# %s, torch %s; configs[1]: %s; %d windows of %d calls"
        % (torch.cuda.get_device_name(0), torch.__version__, {k: c[k] for k in ("B", "Ts", "Tt", "H", "V")}, a.windows, a.iters))
    src, lens, tgt, im = bench.make_batch(c, 0, dev)
    lt = torch.tensor(lens, dtype=torch.int32, device=dev)
    this = _lib.lib()
    models = [bench.build_model(c, dev, seed=1234 + i, dropout=False).eval() for i in range(3)]
    B, Tt, V = c["B"], c["Tt"], c["V"]

    # 1. the whole call
    for M in (1, 3):
        obj = models[0] if M == 1 else Ensemble(models[:M])
        s = row("M=%d score_translations" % M, windows(lambda: obj.score_translations(src, lt, tgt, im), a.windows, a.iters, warmup=5))
        t = row("M=%d token_confidence" % M, windows(lambda: obj.token_confidence(src, lt, tgt, im), a.windows, a.iters, warmup=5))
        say("#   M=%d: token_confidence - score_translations = %+.4f ms (%+.2f %%)" % (M, t - s, 100.0 * (t - s) / s))

    # 2. the row kernel against its bytes
    full = torch.randint(4, V, (B, Tt), device=dev)              # every position in the span
    none = torch.zeros(B, Tt, dtype=torch.int64, device=dev)     # no position in the span: launch + span scans + the sentence kernel
    tg, tok = scoring.forced_args(models, [True] * 3, src, tgt, im)
    with torch.no_grad():
        outs = [scoring._member_logits(m, src, lt, im, tok, tg) for m in models]
    o = confidence._conf_call(outs[:1], tg, V)
    bufs = [o.token_logp, o.entropy, o.rank, o.top, o.top_logp, o.sentence]

    def conf_call(M, y):
        _lib.call("vag_token_conf", (C.c_void_p * M)(*[ptr(x[0]) for x in outs[:M]]), (C.c_int64 * M)(*[x[0].shape[1] for x in outs[:M]]),
                  (C.c_void_p * M)(*[ptr(x[1]) for x in outs[:M]]), M, ptr(y, torch.int64), B, Tt, V, ptr(bufs[0]), ptr(bufs[1]),
                  ptr(bufs[2], torch.int32), ptr(bufs[3], torch.int32), ptr(bufs[4]), ptr(bufs[5]), stream())
    for M in (1, 3):
        empty = row("M=%d vag_token_conf, all-pad targets (no row read)" % M, windows(lambda: conf_call(M, none), a.windows, 10 * a.iters))
        for what, y in (("every position in the span", full), ("the batch's targets", tg)):
            n = int(confidence._conf_call(outs[:1], y, V).sentence[:, 2].sum())
            t = row("M=%d vag_token_conf, %s" % (M, what), windows(lambda: conf_call(M, y), a.windows, 10 * a.iters))
            nbytes = M * n * V * 4
            say("#   %d span rows of %d: %.1f MB read once; %.1f us -> %.2f TB/s (less the all-pad call's %.1f us: %.2f TB/s)"
                % (n, B * Tt, nbytes / 1e6, 1e3 * t, nbytes / (t * 1e-3) / 1e12, 1e3 * empty,
                   nbytes / (max(t - empty, 1e-6) * 1e-3) / 1e12))

    # 3. the unchanged paths, this build against the parent's library
    configs = [("this build", this)]
    if a.parent_lib:
        configs.insert(0, ("parent    ", load_parent(a.parent_lib)))
    medians = {}
    for rnd in range(a.rounds):
        for what, L in configs:
            _lib._lib = L                        # every call below goes to this library
            try:
                m = bench.build_model(c, dev, dropout=False).eval()
                ws = windows(lambda: m.score_translations(src, lt, tgt, im), a.windows, a.iters, warmup=5)
                wb = windows(lambda: m.beamsearch_decode(src, lens, im, 12, 40), a.windows, max(2, a.iters // 5), warmup=3)
                del m
            finally:
                _lib._lib = this
            medians.setdefault((what, "score_translations"), []).append(row("round %d  %s score_translations" % (rnd + 1, what), ws))
            medians.setdefault((what, "beamsearch_decode"), []).append(row("round %d  %s beamsearch_decode k=12" % (rnd + 1, what), wb))
    say("# means of the rounds' medians:")
    for (what, call), v in medians.items():
        base = statistics.mean(medians[("this build", call)])
        say("#   %s %-20s %.4f ms  (%+.4f ms, %+.2f %% against this build)"
            % (what, call, statistics.mean(v), statistics.mean(v) - base, 100.0 * (statistics.mean(v) - base) / base))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

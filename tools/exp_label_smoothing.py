"""Cost of label smoothing at BASELINE configs[1] size (B=64, Ts=Tt=40, H=512, V=9391): the whole optimiser step (TrainStep.step,
graph replay, train mode) and the output head's forward + backward alone (vag_head_ce_seq_fwd_ls + _bwd_ls on private
buffers), each at eps = 0 and eps = 0.1 from the same build in the same process.  Warm-up, then timed windows of back-to-back
launches between two events; the median window is reported.

    python tools/exp_label_smoothing.py [--windows 7] [--iters 50] >> profiles/exp_label_smoothing.txt

Per-kernel times: run this script under `rocprofv3 --kernel-trace --stats -- python tools/exp_label_smoothing.py --iters 20`
and read the lse_nll_kernel<40, false|true> and ce_bwd_colsum_kernel<false|true> rows of the kernel statistics."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vag-nmt_amd")]

import torch  # noqa: E402


def windows(fn, n_windows, iters, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    import bench
    from machine_translation_vision.losses import LabelSmoothedNLLLoss, PairwiseRankingLoss
    from vagnmt_hip._lib import HeadW, call, ptr, stream
    from vagnmt_hip.trainer import TrainStep
    c = bench.CFG2
    dev = torch.device("cuda", 0)
    print("# %s, torch %s; configs[1]: %s" % (torch.cuda.get_device_name(0), torch.__version__, {k: c[k] for k in ("B", "Ts", "Tt", "H", "V")}))
    vw = torch.ones(c["V"], device=dev)
    vw[0] = 0
    batch = bench.make_batch(c, 0, dev)
    src, lens, tgt, im = batch
    lt = torch.tensor(lens, dtype=torch.int32, device=dev)
    for eps, crit in ((0.0, torch.nn.NLLLoss(weight=vw, reduction="none")), (0.0, LabelSmoothedNLLLoss(vw, 0.0)),
                      (0.1, LabelSmoothedNLLLoss(vw, 0.1))):
        m = bench.build_model(c, dev, dropout=True)
        ts = TrainStep(m, crit, PairwiseRankingLoss(margin=0.1), lr=4e-4, weight_decay=1e-5, clip=1.0, teacher_force_ratio=1.0)
        w = windows(lambda: ts.step(src, lt, tgt, im, teacher=True), a.windows, a.iters)
        ts.check()
        print("step  %-22s eps=%.1f  median %.4f ms  (windows %s)" % (type(crit).__name__, eps, statistics.median(w),
                                                                       " ".join("%.4f" % x for x in w)))
        del ts, m
    # the head alone
    B, Tt, E, H, V = c["B"], c["Tt"], c["E"], c["H"], c["V"]
    R, ldl = B * Tt, (V + 3) // 4 * 4
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s, k=1.0: torch.randn(*s, device=dev, generator=g) * k      # noqa: E731
    h2, cc, e = r(Tt, B, H), r(Tt, B, 2 * H), r(Tt, B, E)
    head = [r(E, H, k=0.05), r(E, k=0.1), r(E, 2 * H, k=0.05), r(E, k=0.1), r(E, E, k=0.05), r(E, k=0.1), r(V, E, k=0.1), r(V, k=0.1)]
    grads = [torch.zeros_like(t) for t in head]
    z = lambda *s: torch.zeros(*s, device=dev)      # noqa: E731
    tmid, logits, lse, nll, inv, loss = z(R, E), z(R, ldl), z(R), z(R), z(B), z(1)
    d_h2, d_c, d_e, scr, one = z(R, H), z(R, 2 * H), z(R, E), z(R * E), torch.ones(1, device=dev)
    hw, hg = HeadW(*[ptr(t) for t in head]), HeadW(*[ptr(t) for t in grads])
    for eps in (0.0, 0.1):
        def fb():
            call("vag_head_ce_seq_fwd_ls", ptr(h2), ptr(cc), ptr(e), hw, ptr(tgt, torch.int64), ptr(vw), B, Tt, E, H, V, 0.0, None, 0,
                 ptr(tmid), ptr(logits), ldl, ptr(lse), ptr(nll), ptr(inv), ptr(loss), eps, stream())
            call("vag_head_ce_seq_bwd_ls", ptr(h2), ptr(cc), ptr(e), hw, ptr(tgt, torch.int64), ptr(vw), B, Tt, E, H, V, 0.0, None,
                 ptr(tmid), ptr(logits), ldl, ptr(lse), ptr(inv), ptr(one), ptr(d_h2), ptr(d_c), ptr(d_e), hg, ptr(scr), eps, stream())
        w = windows(fb, a.windows, a.iters)
        print("head  fwd_ls + bwd_ls        eps=%.1f  median %.4f ms  (windows %s)  loss_mt %.5f" %
              (eps, statistics.median(w), " ".join("%.4f" % x for x in w), float(loss)))


if __name__ == "__main__":
    main()

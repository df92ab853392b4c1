"""Every vag_beam_*_step entry, host and _dev form, on the same seeded inputs under two builds of the library, each in a fresh child
process; every output byte compared.  Usage: python tools/exp_beam_refactor_bits.py PARENT_LIB BRANCH_LIB OUT.txt (GPU box; fails without a GPU)"""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEN = 5
EOS = 3


def worker(lib, out):
    os.environ["VAG_LIB"] = lib
    sys.path.insert(0, os.path.join(ROOT, "vag-nmt_amd"))
    import numpy as np
    import torch
    from vagnmt_hip import _lib
    L = _lib.lib()
    I32, I64 = torch.int32, torch.int64
    res = {}

    def pp(ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def p64(v):
        return (C.c_int64 * len(v))(*v)

    def stream():
        return _lib.stream()

    def inputs(seed, B, k, V, ldl, M, Hs, quant):
        """per step: logp per member (rows, ldl), h_in per member (rows, H)"""
        g = torch.Generator().manual_seed(seed)
        steps = []
        for di in range(MAX_LEN + 1):
            rows = B * (1 if di == 0 else k)
            lps, hs = [], []
            for m in range(M):
                x = torch.randn(rows, V, generator=g) * 2.0
                boost = torch.rand(rows, generator=g) < 0.3
                x[:, EOS] += boost.float() * 9.0
                x = torch.log_softmax(x, 1)
                if quant:
                    x = torch.round(x * 4.0) / 4.0
                full = torch.full((rows, ldl), 100.0)
                full[:, :V] = x
                lps.append(full.cuda())
                hs.append(torch.randn(rows, Hs[m], generator=g).cuda())
            steps.append((lps, hs))
        return steps, g

    def run(tag, kind, B, k, V, ldl, M, flags, extra, seed, quant):
        Hs = [8, 12, 6][:M]
        steps, g = inputs(seed, B, k, V, ldl, M, Hs, quant)
        Tp = extra.get("Tp", 9)
        side = {}
        if kind == "pen":
            side["cp_row"] = [(-torch.rand(B * k, generator=g)).cuda() for _ in range(MAX_LEN + 1)]
            side["cov_row"] = [torch.rand(B * k, Tp, generator=g).cuda() for _ in range(MAX_LEN + 1)]
            Ls = torch.arange(MAX_LEN + 1, dtype=torch.float32)
            side["lp"] = (((5.0 + Ls) / 6.0) ** 0.6).cuda()
            side["bonus"] = (0.1 * Ls).cuda()
        if kind == "req":
            table = torch.zeros(B, 16, 8, dtype=I64)
            for b in range(B - 1):
                for c in range(3 + b):
                    n = 1 + (b + c) % 3
                    table[b, c, :n] = torch.randint(4, min(V, 40), (n,), generator=g)
            side["table"] = table.cuda()
        if kind == "logits":
            nparts = 3
            side["nparts"] = nparts
        for form in ("host", "dev"):
            beam = torch.zeros(2 * MAX_LEN, B, k, dtype=I64, device="cuda")
            nll = torch.zeros(B, k, device="cuda")
            n_alive = torch.full((1,), -7, dtype=I32, device="cuda")
            name = {"ens": "vag_beam_scratch_bytes", "one": "vag_beam_scratch_bytes", "logits": "vag_beam_scratch_bytes",
                    "div": "vag_beam_div_scratch_bytes", "req": "vag_beam_req_scratch_bytes", "sbs": "vag_beam_sbs_scratch_bytes",
                    "pen": "vag_beam_pen_scratch_bytes"}[kind]
            scratch = torch.zeros(getattr(L, name)(B, k, V, MAX_LEN), dtype=torch.uint8, device="cuda")
            tok = torch.full((B * k,), -1, dtype=I64, device="cuda")
            di_state = torch.zeros(2, dtype=I32, device="cuda")
            carried = {}
            if kind == "sbs":
                carried["gum"] = torch.full((B, k), float("nan"), device="cuda")
                rng = torch.tensor([seed, 2], dtype=I64, device="cuda")
            if kind == "req":
                carried["req_state"] = torch.zeros(B, k, 4, dtype=I32, device="cuda")
            if kind == "pen":
                carried["lens"] = torch.zeros(B, k, dtype=I32, device="cuda")
                carried["cpen"] = torch.zeros(B, k, device="cuda")
                carried["cov"] = torch.zeros(B, k, Tp, device="cuda")
            nsteps = MAX_LEN + (1 if form == "dev" else 0)        # the _dev form once past the end: nothing may move
            for di in range(nsteps):
                dev_form = form == "dev" and di > 0
                lps, hs = steps[di]
                rows = lps[0].shape[0]
                h_out = [torch.full((B * k, H), float("nan"), device="cuda") for H in Hs]
                if dev_form and di == 1:
                    di_state.copy_(torch.tensor([1, 0], dtype=I32))
                dargs = (di_state.data_ptr(), MAX_LEN) if dev_form else (di, MAX_LEN)
                targs = (tok.data_ptr(),) if dev_form else ()
                sfx = "_dev" if dev_form else ""
                if kind == "one":          # the single-model entries
                    fn = "vag_beam_step%s%s" % (sfx, "_opt" if flags else "")
                    args = (lps[0].data_ptr(), ldl, nll.data_ptr(), beam.data_ptr(), *dargs, hs[0].data_ptr(), h_out[0].data_ptr(), *targs,
                            B, k, V, Hs[0], n_alive.data_ptr(), scratch.data_ptr()) + ((flags,) if flags else ()) + (stream(),)
                elif kind == "logits":
                    if not dev_form:       # step 0 / the host sequence: the log-probability entry on normalised rows
                        fn = "vag_beam_step_opt"
                        args = (lps[0].data_ptr(), ldl, nll.data_ptr(), beam.data_ptr(), *dargs, hs[0].data_ptr(), h_out[0].data_ptr(),
                                B, k, V, Hs[0], n_alive.data_ptr(), scratch.data_ptr(), flags, stream())
                    else:
                        npt = side["nparts"]
                        x = lps[0][:, :V]
                        cuts = [0, V // 3, 2 * V // 3, V]
                        parts = torch.empty(npt, rows, 2, device="cuda")
                        for q in range(npt):
                            seg = x[:, cuts[q]:cuts[q + 1]]
                            mx = seg.max(1).values
                            parts[q, :, 0] = mx
                            parts[q, :, 1] = torch.exp(seg - mx[:, None]).sum(1)
                        fn = "vag_beam_step_logits_dev_opt"
                        args = (lps[0].data_ptr(), ldl, parts.data_ptr(), npt, nll.data_ptr(), beam.data_ptr(), *dargs, hs[0].data_ptr(),
                                h_out[0].data_ptr(), *targs, B, k, V, Hs[0], n_alive.data_ptr(), scratch.data_ptr(), flags, stream())
                else:
                    pre = (pp(lps), p64([ldl] * M), M, nll.data_ptr(), beam.data_ptr(), *dargs, pp(hs), pp(h_out), p64(Hs), *targs, B, k, V,
                           n_alive.data_ptr(), scratch.data_ptr())
                    if kind == "ens":
                        fn = "vag_beam_ens_step%s%s" % (sfx, "_opt" if flags else "")
                        args = pre + ((flags,) if flags else ()) + (stream(),)
                    elif kind == "div":
                        fn = "vag_beam_div_step" + sfx
                        args = pre + (flags, extra["G"], extra["lam"], stream())
                    elif kind == "req":
                        fn = "vag_beam_req_step" + sfx
                        args = pre + (flags, side["table"].data_ptr(), carried["req_state"].data_ptr(), stream())
                    elif kind == "sbs":
                        fn = "vag_beam_sbs_step" + sfx
                        args = pre + (flags, rng.data_ptr(), carried["gum"].data_ptr(), stream())
                    else:
                        fn = "vag_beam_pen_step" + sfx
                        cover = extra["cover"]
                        cpr = side["cp_row"][di][:rows].contiguous()       # (alive until the synchronise below)
                        cvr = side["cov_row"][di][:rows].contiguous()
                        args = pre + (flags, carried["lens"].data_ptr(), cpr.data_ptr(), carried["cpen"].data_ptr(),
                                      cvr.data_ptr() if cover else None, carried["cov"].data_ptr() if cover else None, Tp,
                                      side["lp"].data_ptr(), side["bonus"].data_ptr(), extra["stepwise"], stream())
                rc = getattr(L, fn)(*args)
                torch.cuda.synchronize()
                assert rc == 0, (tag, form, di, fn, rc)
                key = "%s|%s|step%d|" % (tag, form, di)
                res[key + "beam"] = beam.cpu().numpy().copy()
                res[key + "nll"] = nll.cpu().numpy().view(np.int32).copy()
                res[key + "n_alive"] = n_alive.cpu().numpy().copy()
                res[key + "tok_out"] = tok.cpu().numpy().copy()
                res[key + "di_state"] = di_state.cpu().numpy().copy()
                for m, h in enumerate(h_out):
                    res[key + "h_out%d" % m] = h.cpu().numpy().view(np.int32).copy()
                for nm, t in carried.items():
                    a = t.cpu().numpy()
                    res[key + nm] = (a.view(np.int32) if a.dtype == np.float32 else a).copy()
                if di >= MAX_LEN:
                    break
                # the next step's scores continue from this one's (the library wrote nll); nothing else to feed

    seed = 100
    DIV = [(3, 6, 3, 50, 50), (2, 4, 4, 2500, 2504), (1, 12, 2, 4100, 4100), (2, 64, 8, 70, 70), (2, 12, 3, 10000, 10000)]
    for B, k, G, V, ldl in DIV:
        for M in (1, 3):
            for flags in (0, 3):
                seed += 1
                q = seed % 2 == 0
                shape = "B%d_k%d_V%d_ldl%d_M%d_f%d" % (B, k, V, ldl, M, flags)
                run("ens|" + shape, "ens", B, k, V, ldl, M, flags, {}, seed, q)
                run("div_G%d|" % G + shape, "div", B, k, V, ldl, M, flags, dict(G=G, lam=0.5), seed, q)
                for sw in (0, 1):
                    for cover, Tp in ((True, 9), (True, 8), (False, 9)):
                        run("pen_sw%d_cov%d_Tp%d|" % (sw, cover, Tp) + shape, "pen", B, k, V, ldl, M, flags,
                            dict(stepwise=sw, cover=cover, Tp=Tp), seed, q)
        for flags in (0, 2):
            seed += 1
            shape = "B%d_k%d_V%d_ldl%d_M1_f%d" % (B, k, V, ldl, flags)
            run("one|" + shape, "one", B, k, V, ldl, 1, flags, {}, seed, True)
            if V >= 2048:
                run("logits|" + shape, "logits", B, k, V, ldl, 1, flags, {}, seed, False)
    for k in (1, 5, 12):
        for V in (37, 2048 + 37, 14400):
            for M in (1, 3):
                for flags in (0, 3):
                    seed += 1
                    run("sbs|B3_k%d_V%d_M%d_f%d" % (k, V, M, flags), "sbs", 3, k, V, V + 3, M, flags, {}, seed, seed % 2 == 0)
    for B, k, V, ldl in [(2, 3, 37, 40), (3, 5, 2500, 2501), (3, 16, 18000, 18000)]:
        for M in (1, 3):
            for flags in (0, 3):
                seed += 1
                run("req|B%d_k%d_V%d_M%d_f%d" % (B, k, V, M, flags), "req", B, k, V, ldl, M, flags, {}, seed, seed % 2 == 0)
    np.savez(out, **res)
    print("worker %s: %d arrays" % (lib, len(res)))


def main():
    parent, branch, out = sys.argv[1:4]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    files = []
    for side, lib in (("parent", parent), ("branch", branch)):
        f = os.path.join(os.path.dirname(os.path.abspath(out)), "bitid_%s.npz" % side)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", os.path.abspath(lib), f], timeout=420)
        if r.returncode != 0:
            print("worker for %s failed with %d: stopping" % (side, r.returncode))
            return r.returncode or 1
        files.append(f)
    import numpy as np
    a, b = np.load(files[0]), np.load(files[1])
    assert sorted(a.files) == sorted(b.files)
    bad, nbytes = [], 0
    per = {}
    for key in a.files:
        same = a[key].tobytes() == b[key].tobytes() and a[key].dtype == b[key].dtype
        nbytes += a[key].nbytes
        kind = key.split("|")[0].split("_")[0] + "/" + key.split("|")[2] + "/" + key.split("|")[-1].rstrip("0123456789")
        per.setdefault(kind, [0, 0])
        per[kind][0] += 1
        per[kind][1] += 0 if same else 1
        if not same:
            bad.append(key)
    # sanity: the runs did something (selections moved, alive counts counted, some rows finished)
    moved = sum(int(a[k].any()) for k in a.files if k.endswith("|beam"))
    alive = sorted({int(a[k][0]) for k in a.files if k.endswith("|n_alive")})
    lines = ["bit identity, parent library against branch library: %d arrays, %d bytes, %d differ" % (len(a.files), nbytes, len(bad)),
             "beam buffers that hold something: %d; distinct alive counts seen: %d (min %d, max %d)" % (moved, len(alive), alive[0], alive[-1])]
    for kind in sorted(per):
        lines.append("  %-28s arrays %5d  differing %d" % (kind, per[kind][0], per[kind][1]))
    lines += ["DIFFERS: " + k for k in bad[:40]]
    text = "\n".join(lines)
    print(text)
    with open(out, "w") as f:
        f.write(text + "\n")
    for f in files:
        os.remove(f)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--worker":
        worker(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main())

"""Record tests/golden/gemm_plans.json: the single-product planner's (T, split-K) per product, read from the "[vag_gemm]" line a
`make LAB=1` library prints under vag_set_option("gemm_debug", 1).  No device is needed: the line is printed before the launch,
which then fails with hipErrorNoDevice on a machine without one.  The pointers handed over are never dereferenced on the host.

    python tools/record_gemm_plans.py path/to/libvagnmt_lab.so > tests/golden/gemm_plans.json

The committed file was recorded from the library of the commit BEFORE the planner was made a function of its own
(tests/test_gemm_plan_host.py holds vag_gemm_plan to it); re-record only from a library whose choices are known to be the wanted ones.
"""
import ctypes as C
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPTS = ("gemm_force_tile", "gemm_force_splitk", "gemm_f32mfma")
# the dense products of one configs[1] training step (profiles/r03_exp_gemm_shapes.txt, DESIGN.md product table)
STEP_SHAPES = [("head_logits", 2560, 9391, 256), ("attn_keys", 2560, 1024, 1024), ("enc_in_proj", 2560, 1536, 256),
               ("encwp", 2560, 1536, 1024), ("d_tmid", 2560, 256, 9391), ("d_out_weight", 9391, 256, 2560),
               ("g_W_hh", 1536, 512, 2560), ("g_wcat", 2560, 512, 2560), ("g_attn_e", 1024, 1024, 2560),
               ("d_enc", 2560, 1024, 1024)]
LAYOUTS = [(1, 1), (1, 0), (0, 1), (0, 0)]


def cases():
    """(id, M, N, K, a_kc, b_kc, vec, beta, act, storage, options)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gemm_paths", os.path.join(ROOT, "tests", "test_gpu_gemm_paths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = []
    for name, M, N, K, kw in mod.GEMM_CASES:
        opts = {k: int(kw[k]) for k in OPTS if k in kw}
        for a_kc, b_kc in LAYOUTS:
            out.append((name, M, N, K, a_kc, b_kc, 0 if kw.get("off", 0) else 1, float(kw.get("beta", 0.0)), int(kw.get("act", 0)), 0, opts))
    for storage in (0, 1):
        for name, M, N, K in STEP_SHAPES:
            for beta in (0.0, 1.0):
                for a_kc, b_kc in LAYOUTS:
                    out.append(("step_" + name, M, N, K, a_kc, b_kc, 1, beta, 0, storage, {}))
    return out


def main():
    L = C.CDLL(sys.argv[1])
    I64, F, P = C.c_int64, C.c_float, C.c_void_p
    L.vag_gemm_f32.argtypes = [I64, I64, I64, F, P, I64, I64, P, I64, I64, F, P, I64, P, C.c_int, P]
    L.vag_set_option.argtypes = [C.c_char_p, I64]
    L.vag_set_operator_context.argtypes = [P, C.c_int]
    assert L.vag_set_option(b"gemm_debug", 1) == 0, "not a LAB=1 library"
    todo = cases()
    log = tempfile.TemporaryFile()
    keep = os.dup(2)
    os.dup2(log.fileno(), 2)
    try:
        for _, M, N, K, a_kc, b_kc, vec, beta, act, storage, opts in todo:
            for k in OPTS:
                L.vag_set_option(k.encode(), opts.get(k, 0))
            L.vag_set_operator_context(P(4096) if storage else None, storage)
            ld = lambda inner: (inner + 3) // 4 * 4 + 4        # noqa: E731  (tests/test_gpu_gemm_paths.py: _ld)
            base = 1 << 20
            A = base + (0 if vec else 4)
            sam, sak = (ld(K), 1) if a_kc else (1, ld(M))
            sbk, sbn = (1, ld(K)) if b_kc else (ld(N), 1)
            L.vag_gemm_f32(M, N, K, 1.0, P(A), sam, sak, P(A + (1 << 30)), sbk, sbn, beta, P(base + (1 << 31)), N + 5, None, act, None)
    finally:
        os.dup2(keep, 2)
    log.seek(0)
    lines = [l for l in log.read().decode().splitlines() if l.startswith("[vag_gemm]")]
    assert len(lines) == len(todo), (len(lines), len(todo))
    rec = []
    for (name, M, N, K, a_kc, b_kc, vec, beta, act, storage, opts), l in zip(todo, lines):
        m = re.match(r"\[vag_gemm\] M=(\d+) N=(\d+) K=(\d+) akc=(\d) bkc=(\d) beta=(\S+) -> T=(\d+) splitk=(\d+) ", l)
        assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5))) == (M, N, K, a_kc, b_kc), l
        rec.append(dict(id=name, M=M, N=N, K=K, a_kc=a_kc, b_kc=b_kc, vec=vec, beta=beta, act=act, storage=storage, opts=opts,
                        T=int(m.group(7)), splitk=int(m.group(8))))
    print("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rec) + "\n]")


if __name__ == "__main__":
    main()

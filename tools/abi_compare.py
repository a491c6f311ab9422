"""Byte-for-byte comparison of two builds of libgp_predict_hip.so through the C ABI: the instrument for a
change of the host layer that must leave every result, return code and message as it was.

    GP_PREDICT_LIB=old.so python tools/abi_compare.py dump --out old.pkl [--gpu]
    python tools/abi_compare.py dump --out new.pkl [--gpu]
    python tools/abi_compare.py compare old.pkl new.pkl

``dump`` runs a fixed, seeded set of calls on the library GP_PREDICT_LIB selects (default: the in-tree build)
and saves every output array, return code and error string.  Each part runs in a child process of its own --
the launch plans once per environment switch, several of which the library reads once per process -- so a
process loads one library, never two.  Without ``--gpu`` no call touches a device.  ``compare`` demands byte
equality, record by record, and lists what differs (the file:line a failed HIP call appends is left out).
"""
import argparse, ctypes, itertools, os, pickle, re, subprocess, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32, F64 = 0, 1
NP = {F32: np.float32, F64: np.float64}
SHAPES = [(3, 1), (16, 2), (17, 4), (37, 3), (250, 10), (300, 16), (321, 16), (20, 17)]
PLAN_ENVS = [None, "GP_NO_FEW=1", "GP_HESS_VALU=1", "GP_RECON_WIDE=0", "GP_RECON_WIDE=1", "GP_NO_KSKIP=1"]
c_int, c_i64, byref = ctypes.c_int, ctypes.c_int64, ctypes.byref
RECORDS = []
lib = None


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def rec(label, rc, *outs):
    """One call: its status, its message when it failed, and the bytes of every output."""
    err = lib.gp_last_error_string().decode() if rc not in (0, 1) else ""
    RECORDS.append((label, int(rc), err, [np.ascontiguousarray(o).tobytes() for o in outs]))


def emulator(N, D, E=1, seed=0):
    """Seeded constants of E emulators on shared inputs, float64: expX [E][D+2], inputs, invQt [E][N], invQ [E][N][N]."""
    r = np.random.RandomState(1000 * N + 10 * D + seed)
    expX = np.concatenate([r.uniform(0.5, 2.0, (E, D)), r.uniform(1.0, 1.5, (E, 1)), np.full((E, 1), 1e-3)], axis=1)
    a = r.standard_normal((E, N, N)) / np.sqrt(N)
    return expX, r.uniform(0, 1, (N, D)), r.standard_normal((E, N)), a @ a.transpose(0, 2, 1) + np.eye(N)


def dump_cpu():
    for dt in (F32, F64):
        rows, msgs = [], []
        for N, D in itertools.product(range(1, 331), range(1, 19)):
            kd, knb, ks, xa, fr = c_int(-9), c_int(-9), c_int(-9), c_i64(-9), c_i64(-9)
            rc = lib.gp_pack_sizes(dt, N, D, byref(kd), byref(knb), byref(xa), byref(fr))
            if rc: msgs.append(lib.gp_last_error_string().decode())
            rc2 = lib.gp_kernel_ksteps(N, D, byref(ks))
            if rc2: msgs.append(lib.gp_last_error_string().decode())
            rows.append((rc, kd.value, knb.value, xa.value, fr.value, rc2, ks.value))
        rec("pack_sizes+ksteps dtype=%d" % dt, 0, np.array(rows, np.int64), np.array("\n".join(msgs).encode()))
    for (N, D), dt, with_q in itertools.product(SHAPES, (F32, F64), (True, False)):
        expX, inputs, invQt, invQ = [x.astype(NP[dt]) for x in emulator(N, D)]
        kd, knb, xa_len, fr_len = c_int(), c_int(), c_i64(), c_i64()
        lib.gp_pack_sizes(dt, N, D, byref(kd), byref(knb), byref(xa_len), byref(fr_len))
        xa, fr = np.zeros(xa_len.value, NP[dt]), np.zeros(fr_len.value, NP[dt])
        sd, b = np.zeros(2 * kd.value + 1, NP[dt]), np.zeros(1, NP[dt])
        fn = lib.gp_pack_model_f64 if dt == F64 else lib.gp_pack_model_f32
        rc = fn(P(expX[0]), P(inputs), P(invQt[0]), P(invQ[0]) if with_q else None, N, D, D + 2, P(xa),
                P(fr) if with_q else None, P(sd), P(b))
        rec("pack_model N=%d D=%d dtype=%d invQ=%d" % (N, D, dt, with_q), rc, xa, fr, sd, b)
    rec("pack_model null", lib.gp_pack_model_f64(*([None] * 4 + [3, 1, 3] + [None] * 4)))
    rec("frag_index NB=7", 0, np.array([lib.gp_frag_index(7, I, J, s) for I in range(-1, 8) for J in range(-1, 8)
                                        for s in range(-1, 5)], np.int64))
    r = np.random.RandomState(5)
    blocks = [r.bytes(n) for n in (1, 4099, 250 * 250 * 8)]
    ptrs = (ctypes.c_char_p * 3)(*blocks)
    lens = (c_i64 * 3)(*[len(b) for b in blocks])
    rec("content_digest", 0, np.array([lib.gp_content_digest(ptrs, lens, k) for k in (0, 1, 2, 3)], np.uint64))


def dump_plan(tag):
    rows, msgs = [], []
    for op, dt, (N, D), E, M, al in itertools.product(range(6), (F32, F64), SHAPES, (1, 3), (1, 64, 65, 4099, 1000000), (0, 1)):
        k, wg, rwg, rpi, it, rit = c_int(-9), c_int(-9), c_int(-9), c_int(-9), c_i64(-9), c_i64(-9)
        rc = lib.gp_launch_plan(op if op < 5 else 99, dt, N, D, E, M, N, 256, al, byref(k), byref(it), byref(wg), byref(rit),
                                byref(rwg), byref(rpi))
        if rc: msgs.append(lib.gp_last_error_string().decode())
        rows.append((rc, k.value, it.value, wg.value, rit.value, rwg.value, rpi.value))
    ks = c_int(-9)      # (the kernel choice itself has a switch of its own)
    steps = [(lib.gp_kernel_ksteps(N, 2, byref(ks)), ks.value) for N in range(1, 331)]
    rec("launch_plan env=%s" % tag, 0, np.array(rows, np.int64), np.array(steps, np.int64), np.array("\n".join(msgs).encode()))


class Gpu:
    """A context and what the GPU part needs of it: device buffers, pinned arrays, models."""

    def __init__(self):
        self.ctx = ctypes.c_void_p()
        rc = lib.gp_ctx_create(0, byref(self.ctx))
        if rc: raise SystemExit("gp_ctx_create: " + lib.gp_last_error_string().decode())

    def dev(self, nbytes):
        p = ctypes.c_void_p()
        assert lib.gp_malloc(self.ctx, max(int(nbytes), 16), byref(p)) == 0
        assert lib.gp_memset(self.ctx, p, 0, max(int(nbytes), 16)) == 0
        return p

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.dev(a.nbytes)
        if a.nbytes: assert lib.gp_memcpy_h2d(self.ctx, p, P(a), a.nbytes) == 0
        return p

    def down(self, p, n, dtype):
        a = np.zeros(n, dtype)
        if a.nbytes: assert lib.gp_memcpy_d2h(self.ctx, P(a), p, a.nbytes) == 0
        else: lib.gp_ctx_synchronize(self.ctx)
        return a

    def pinned(self, n, dtype, init=None):
        p = ctypes.c_void_p()
        nbytes = max(1, n * np.dtype(dtype).itemsize)
        assert lib.gp_pinned_alloc(self.ctx, nbytes, byref(p)) == 0
        a = np.frombuffer((ctypes.c_char * nbytes).from_address(p.value), np.uint8)[:n * np.dtype(dtype).itemsize].view(dtype)
        if init is not None: a[:] = init.ravel()
        return a

    def model(self, N, D, E, cdt, hdt):
        consts = [np.ascontiguousarray(x.astype(NP[hdt])) for x in emulator(N, D, E)]
        fn = {(F64, F64): lib.gp_batch_create_f64, (F32, F32): lib.gp_batch_create_f32,
              (F32, F64): lib.gp_batch_create_f32_h64}[(cdt, hdt)]
        m = ctypes.c_void_p()
        rc = fn(self.ctx, E, P(consts[0]), P(consts[1]), P(consts[2]), P(consts[3]), N, D, D + 2, byref(m))
        rec("batch_create N=%d D=%d E=%d c=%d h=%d" % (N, D, E, cdt, hdt), rc)
        return m, consts


def dump_gpu():
    g = Gpu()
    ctx = g.ctx
    PAIRS = [(F64, F64), (F32, F32), (F32, F64)]
    for (N, D, E), (cdt, hdt) in itertools.product([(37, 3, 1), (40, 9, 1), (20, 17, 1), (40, 9, 3)], PAIRS):
        m, consts = g.model(N, D, E, cdt, hdt)
        T, TH, tag = NP[cdt], NP[hdt], "N=%d D=%d E=%d c=%d h=%d" % (N, D, E, cdt, hdt)
        for M in (83, 1, 0):
            y = np.random.RandomState(M).uniform(0, 1, (M, D))
            yh, yd, tm = y.astype(TH), g.up(y.astype(T)), "%s M=%d" % (tag, M)
            for layout, blk in itertools.product((0, 1), (0, 32)):
                mu, var, der = np.zeros(E * M, TH), np.zeros(E * M, TH), np.zeros(E * M * D, TH)
                rc = lib.gp_predict_host(ctx, m, hdt, P(yh), P(mu), P(var), P(der), M, layout, blk)
                rec("predict_host %s layout=%d block=%d" % (tm, layout, blk), rc, mu, var, der)
                mu, der = np.zeros(E * M, TH), np.zeros(E * M * D, TH)
                rc = lib.gp_predict_mean_grad_host(ctx, m, hdt, P(yh), P(mu), P(der), M, layout, blk)
                rec("mean_grad_host %s layout=%d block=%d" % (tm, layout, blk), rc, mu, der)
            if cdt == hdt and E == 1:      # page-locked arrays and a block bound: the pinned route
                py, pmu, pvar, pder = g.pinned(M * D, TH, yh), g.pinned(M, TH), g.pinned(M, TH), g.pinned(M * D, TH)
                rc = lib.gp_predict_host(ctx, m, hdt, P(py), P(pmu), P(pvar), P(pder), M, 1, 32)
                rec("predict_host pinned " + tm, rc, pmu, pvar, pder)
                pmu[:], pder[:] = 0, 0
                rc = lib.gp_predict_mean_grad_host(ctx, m, hdt, P(py), P(pmu), P(pder), M, 1, 32)
                rec("mean_grad_host pinned " + tm, rc, pmu, pder)
            if cdt == hdt:                 # device buffers hold the model's dtype
                for layout in (0, 1):
                    d_mu, d_var, d_der = g.dev(E * M * 8), g.dev(E * M * 8), g.dev(E * M * D * 8)
                    rc = lib.gp_predict_device(ctx, m, yd, d_mu, d_var, d_der, M, layout)
                    rec("predict_device %s layout=%d" % (tm, layout), rc, g.down(d_mu, E * M, T), g.down(d_var, E * M, T),
                        g.down(d_der, E * M * D, T))
                    d_mu, d_der = g.dev(E * M * 8), g.dev(E * M * D * 8)
                    rc = lib.gp_predict_mean_grad_device(ctx, m, yd, d_mu, d_der, M, layout)
                    rec("mean_grad_device %s layout=%d" % (tm, layout), rc, g.down(d_mu, E * M, T), g.down(d_der, E * M * D, T))
                d_h = g.dev(E * M * D * D * 8)
                rec("hessian_device " + tm, lib.gp_hessian_device(ctx, m, yd, d_h, M), g.down(d_h, E * M * D * D, T))
                h = np.zeros(E * M * D * D, T)
                rec("hessian_host " + tm, lib.gp_hessian_host(ctx, m, P(y.astype(T)), P(h), M), h)
            h = np.zeros(E * M * D * D, np.float64)
            rec("hessian_host_h64 " + tm, lib.gp_hessian_host_h64(ctx, m, P(y), P(h), M), h)
            if E == 1:                      # the reference's boundary: constants with every call, twice (model cache)
                c = [x[0] if i != 1 else x for i, x in enumerate(consts)]
                names = {(F64, F64): ["gp_predict_wrap_f64", "gp_predict_rows_f64"], (F32, F32): ["gp_predict_wrap_f32", "gp_predict_rows_f32"],
                         (F32, F64): ["gp_predict_rows_f32_h64"]}[(cdt, hdt)]
                for name, k in itertools.product(names, (0, 1)):
                    mu, var, der = np.zeros(M, TH), np.zeros(M, TH), np.zeros(M * D, TH)
                    rc = getattr(lib, name)(ctx, P(c[0]), P(c[1]), P(c[2]), P(c[3]), P(yh), P(mu), P(var), P(der), M, N, D, D + 2)
                    rec("%s %s call=%d" % (name, tm, k), rc, mu, var, der)
                if cdt == hdt:
                    for k in (0, 1):
                        h = np.zeros(M * D * D, TH)
                        rc = (lib.gp_hessian_f64 if cdt == F64 else lib.gp_hessian_f32)(ctx, P(c[0]), P(c[1]), P(c[2]), P(yh), P(h), M, N, D, D + 2)
                        rec("gp_hessian %s call=%d" % (tm, k), rc, h)
            if E > 1:
                dump_batch(g, m, cdt, hdt, M, D, E, y, yd, tm)
        lib.gp_model_destroy(m)
    r = np.random.RandomState(9)
    for dt in (F32, F64):
        basis, coef = r.standard_normal((5, 1025)).astype(NP[dt]), r.standard_normal((5, 65)).astype(NP[dt])
        d_out = g.dev(65 * 1025 * 8)
        rc = lib.gp_reconstruct_device(ctx, dt, g.up(basis), g.up(coef), d_out, 65, 5, 1025)
        rec("reconstruct_device dtype=%d" % dt, rc, g.down(d_out, 65 * 1025, NP[dt]))
    theta, inputs, targets = r.uniform(-1, 1, (2, 5)), r.uniform(0, 1, (9, 3)), r.standard_normal((2, 9))
    for full in (True, False):
        cost, grad, invQ, invQt = np.zeros(2), np.zeros((2, 5)), np.zeros((2, 81)), np.zeros((2, 9))
        rc = lib.gp_likelihood_batch_f64(ctx, 2, P(theta), P(inputs), P(targets), 0, 9, 3, P(cost), P(grad),
                                         P(invQ) if full else None, P(invQt))
        rec("likelihood full=%d" % full, rc, cost, grad, invQ, invQt)
    lib.gp_ctx_destroy(ctx)


def dump_batch(g, m, cdt, hdt, M, D, E, y, yd, tm):
    """Folds over the batch and the multivariate path (the batch as the emulator of 7 bands)."""
    ctx, T, TH, B = g.ctx, NP[cdt], NP[hdt], 7
    r = np.random.RandomState(100 + M)
    w, obs, basis, A = r.uniform(0.5, 1.5, (E, M)), r.standard_normal((E, M)), r.standard_normal((E, B)), r.standard_normal((E, E))
    yh, out = y.astype(TH), np.zeros(M * D * D, TH)
    rec("hessian_weighted_host " + tm, lib.gp_hessian_weighted_host(ctx, m, hdt, P(yh), P(w.astype(TH)), P(out), M), out)
    for shared in (False, True):      # (E, M) observations, or one vector shared by all rows
        o = (obs[:, :1] if shared and M else obs).astype(TH).copy()
        es, ms = (1, 0) if shared else (M, 1)
        cost, grad, wr, gn, hs = np.zeros(M, TH), np.zeros(M * D, TH), np.zeros(E * M, TH), np.zeros(M * D * D, TH), np.zeros(M * D * D, TH)
        rc = lib.gp_band_misfit_host(ctx, m, hdt, P(yh), P(o), es, ms, P(w.astype(TH)), M, 1, P(cost), P(grad), P(wr), P(gn), P(hs), M)
        rec("band_misfit_host %s shared=%d" % (tm, shared), rc, cost, grad, wr, gn, hs)
    if cdt != hdt:
        return
    d_w, d_out = g.up(w.astype(T)), g.dev(M * D * D * 8)
    rec("hessian_weighted_device " + tm, lib.gp_hessian_weighted_device(ctx, m, yd, d_w, d_out, M), g.down(d_out, M * D * D, T))
    d = [g.dev(n * 8) for n in (M, M * D, E * M, M * D * D, M * D * D)]
    rc = lib.gp_band_misfit_device(ctx, m, yd, g.up(obs.astype(T)), M, 1, d_w, M, 1, d[0], d[1], d[2], d[3], d[4], M)
    rec("band_misfit_device " + tm, rc, *[g.down(p, n, T) for p, n in zip(d, (M, M * D, E * M, M * D * D, M * D * D))])
    d_basis, yt, ob, wb, At = g.up(basis.astype(T)), y.astype(T), r.standard_normal((M, B)).astype(T), r.uniform(0.5, 1.5, B).astype(T), A.astype(T)
    blocks = [np.arange(5000, dtype=np.float64), basis.copy()]
    ptrs, lens = (ctypes.c_void_p * 2)(*[b.ctypes.data for b in blocks]), (c_i64 * 2)(*[b.nbytes for b in blocks])
    good = lib.gp_content_digest(ptrs, lens, 2)
    for name, expected in (("plain", None), ("match", good), ("stale", good ^ 1)):
        fwd, jac, res = np.zeros(M * B, T), np.zeros(M * D * B, T), np.zeros(M * (1 + D + E) + M * D * D, T)
        if expected is None:
            rc = lib.gp_mv_predict_host(ctx, m, d_basis, P(yt), M, B, P(fwd), P(jac))
            rc2 = lib.gp_mv_misfit_host(ctx, m, d_basis, P(yt), D, P(ob), B, P(wb), 0, P(At), M, B, P(res))
        else:
            rc = lib.gp_mv_predict_host_checked(ctx, m, d_basis, P(yt), M, B, P(fwd), P(jac), ptrs, lens, 2, expected)
            rc2 = lib.gp_mv_misfit_host_checked(ctx, m, d_basis, P(yt), D, P(ob), B, P(wb), 0, P(At), M, B, P(res), ptrs, lens, 2, expected)
        rec("mv_predict_host %s %s" % (name, tm), rc, fwd, jac)
        rec("mv_misfit_host %s %s" % (name, tm), rc2, res)
    d_mu, d_der = g.dev(E * M * 8), g.dev(E * M * D * 8)
    rec("mean_grad_device for mv " + tm, lib.gp_predict_mean_grad_device(ctx, m, yd, d_mu, d_der, M, 1))
    d = [g.dev(n * 8) for n in (M, E * M, M * D, M * D * D)]
    rc = lib.gp_mv_misfit_device(ctx, cdt, d_basis, d_mu, d_der, g.up(ob), B, g.up(wb), 0, d[0], d[1], d[2], M, E, B, D)
    rec("mv_misfit_device " + tm, rc, *[g.down(p, n, T) for p, n in zip(d, (M, E * M, M * D))])
    rc = lib.gp_mv_gauss_newton_device(ctx, cdt, d_der, g.up(At), d[3], M, E, D)
    rec("mv_gauss_newton_device " + tm, rc, g.down(d[3], M * D * D, T))


def main():
    global lib
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump"); d.add_argument("--out", required=True); d.add_argument("--gpu", action="store_true")
    c = sub.add_parser("compare"); c.add_argument("a"); c.add_argument("b")
    p = sub.add_parser("part"); p.add_argument("what"); p.add_argument("out")      # (dump's children)
    a = ap.parse_args()
    if a.cmd == "part":
        from gp_emulator_amd import _lib
        lib = _lib.load()
        {"cpu": dump_cpu, "gpu": dump_gpu}.get(a.what, lambda: dump_plan(a.what))()
        pickle.dump(RECORDS, open(a.out, "wb"))
    elif a.cmd == "dump":
        records = []
        for what in ["cpu"] + ["plan:%s" % e for e in PLAN_ENVS] + (["gpu"] if a.gpu else []):
            env = dict(os.environ)
            if what.startswith("plan:") and what != "plan:None":
                env.update([what[5:].split("=")])
            tmp = "%s.part" % a.out
            subprocess.run([sys.executable, os.path.abspath(__file__), "part", what.replace("plan:", ""), tmp], env=env, check=True)
            records += pickle.load(open(tmp, "rb"))
            os.remove(tmp)
        pickle.dump(records, open(a.out, "wb"))
        print("%d records -> %s" % (len(records), a.out))
    else:
        A, B = pickle.load(open(a.a, "rb")), pickle.load(open(a.b, "rb"))
        strip = lambda s: re.sub(r" \(\S+:\d+\)$", "", s)
        bad = ["record count %d != %d" % (len(A), len(B))] if len(A) != len(B) else []
        for x, y in zip(A, B):
            if x[0] != y[0]: bad.append("label %r != %r" % (x[0], y[0]))
            elif x[1] != y[1] or strip(x[2]) != strip(y[2]): bad.append("%s: status %d %r != %d %r" % (x[0], x[1], x[2], y[1], y[2]))
            elif x[3] != y[3]: bad.append("%s: output arrays %s differ" % (x[0], [i for i, (p, q) in enumerate(zip(x[3], y[3])) if p != q]))
        print("\n".join(bad) if bad else "identical: %d records, %d bytes of outputs" % (len(A), sum(len(o) for x in A for o in x[3])))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

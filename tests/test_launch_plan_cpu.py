"""gp_launch_plan: how a device call is cut into work items and workgroups, checked without a GPU against
figures written out by hand from the kernel headers' comments (256 compute units, the MI355X):

  predict_kernel          fp64 8 waves = 128 rows per item, fp32 12 waves = 192; one workgroup per CU
  mean+gradient instance  fp64 12 waves = 192 rows, fp32 16 waves = 256; one workgroup per CU
  predict_few_kernel      a workgroup per 16-row tile, up to 2 x compute units tiles
  predict_generic_kernel  16 rows per item, 4 workgroups per CU
  hessian_kernel          4 waves = 64 rows per item, 2 workgroups per CU
  hessian_win_kernel      4 waves = 64 rows per item, 2 workgroups per CU; LDSOUT (KL 3 / KL 4) on the whole
                          64-row groups when n_inputs is the kernel D, its rows are 16-byte pieces and the
                          pointers are aligned, direct stores otherwise and for the rows behind the last group
  reconstruct_kernel      64 rows x one band chunk per item; narrow 256 x 2 vectors (1024 fp64 / 2048 fp32 bands,
                          8 workgroups per CU), wide 512 x 3 (3072 / 6144 bands, 4 per CU); balanced rounds
"""
import numpy as np
import pytest

from gp_emulator_amd import _lib

F64, F32 = np.float64, np.float32
CU = 256


def plan(op, prec, rows, **kw):
    return _lib.launch_plan(op, prec, rows, compute_units=kw.pop("cu", CU), **kw)


def ceil_div(a, b):
    return -(-a // b)


# (op, precision, n_train, n_inputs, n_emulators, rows) -> (kernel, rows_per_item, items, workgroups)
TABLE = [
    # the throughput kernel: one round is 256 items
    (("predict", F64, 250, 11, 1, 32768), ("predict", 128, 256, 256)),
    (("predict", F64, 250, 11, 1, 32769), ("predict", 128, 257, 256)),
    (("predict", F64, 16, 2, 1, 20011), ("predict", 128, 157, 157)),
    (("predict", F32, 300, 16, 1, 49152), ("predict", 192, 256, 256)),
    (("predict", F32, 300, 16, 1, 49153), ("predict", 192, 257, 256)),
    (("mean_grad", F64, 250, 10, 1, 49152 + 1), ("predict", 192, 257, 256)),
    (("mean_grad", F32, 37, 3, 1, 65536 + 1), ("predict", 256, 257, 256)),
    (("mean_grad", F32, 37, 3, 1, 100000), ("predict", 256, 391, 256)),
    # a batch: items are (emulator, row group)
    (("predict", F64, 100, 5, 100, 1037), ("predict", 128, 900, 256)),
    (("predict", F32, 100, 5, 100, 1037), ("predict", 192, 600, 256)),
    (("mean_grad", F64, 192, 13, 100, 1037), ("predict", 192, 600, 256)),
    (("mean_grad", F32, 192, 13, 100, 1037), ("predict", 256, 500, 256)),
    # few rows: a workgroup per 16-row tile
    (("predict", F64, 250, 11, 1, 1), ("predict_few", 16, 1, 1)),
    (("predict", F64, 250, 11, 1, 4099), ("predict_few", 16, 257, 257)),
    (("mean_grad", F32, 250, 11, 12, 100), ("predict_few", 16, 84, 84)),
    # the general-shape kernel: N > 320 or n_inputs > 16
    (("predict", F64, 321, 16, 1, 203), ("generic", 16, 13, 13)),
    (("predict", F32, 640, 30, 1, 16384), ("generic", 16, 1024, 1024)),
    (("mean_grad", F64, 20, 17, 1, 16385), ("generic", 16, 1025, 1024)),
    (("predict", F64, 1024, 64, 1, 40000), ("generic", 16, 2500, 1024)),
    # VALU Hessian: kernel D 2, 4, 5 and every general shape
    (("hessian", F64, 16, 2, 1, 1000), ("hessian_valu", 64, 16, 16)),
    (("hessian", F64, 37, 1, 1, 32768), ("hessian_valu", 64, 512, 512)),
    (("hessian", F32, 17, 3, 1, 32769), ("hessian_valu", 64, 513, 512)),
    (("hessian", F64, 100, 5, 40, 1061), ("hessian_valu", 64, 680, 512)),
    (("hessian", F64, 400, 4, 1, 70000), ("hessian_valu", 64, 1094, 512)),
    (("hessian", F32, 321, 16, 1, 70000), ("hessian_valu", 64, 1094, 512)),
]


@pytest.mark.parametrize("call,want", TABLE)
def test_plan_table(call, want):
    op, prec, n, d, E, rows = call
    p = plan(op, prec, rows, n_train=n, n_inputs=d, n_emulators=E)
    assert (p["kernel"], p["rows_per_item"], p["items"], p["workgroups"]) == want
    assert p["workgroups"] <= p["items"]
    assert (p["rest_items"], p["rest_workgroups"]) == (0, 0)
    assert p["items"] == ceil_div(rows, p["rows_per_item"]) * E


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("op", ["predict", "mean_grad"])
@pytest.mark.parametrize("cu", [256, 304, 8])
def test_few_rows_switch_sits_at_two_tiles_per_compute_unit(op, prec, cu, monkeypatch):
    monkeypatch.delenv("GP_NO_FEW", raising=False)
    edge = 2 * cu * 16
    p = plan(op, prec, edge, n_train=250, n_inputs=11, cu=cu)
    assert (p["kernel"], p["items"], p["workgroups"], p["rows_per_item"]) == ("predict_few", 2 * cu, 2 * cu, 16)
    p = plan(op, prec, edge + 1, n_train=250, n_inputs=11, cu=cu)
    assert p["kernel"] == "predict" and p["rows_per_item"] > 16 and p["workgroups"] <= cu
    # tiles count the emulators of a batch
    assert plan(op, prec, 16 * cu, n_train=250, n_inputs=11, n_emulators=2, cu=cu)["kernel"] == "predict_few"
    assert plan(op, prec, 16 * cu + 1, n_train=250, n_inputs=11, n_emulators=2, cu=cu)["kernel"] == "predict"
    monkeypatch.setenv("GP_NO_FEW", "1")
    p = plan(op, prec, 100, n_train=250, n_inputs=11, cu=cu)
    assert (p["kernel"], p["items"], p["workgroups"]) == ("predict", 1, 1)


@pytest.mark.parametrize("prec", [F64, F32])
def test_windowed_hessian_instances(prec, monkeypatch):
    monkeypatch.delenv("GP_HESS_VALU", raising=False)
    h = lambda n, d, rows, **kw: plan("hessian", prec, rows, n_train=n, n_inputs=d, **kw)
    # KL 3: the block counts of N = 250 and 300 whose last k-step is empty; KL 4 otherwise
    for n, d, kl in ((250, 10, 3), (300, 16, 3), (250, 12, 3), (300, 8, 3), (256, 10, 4), (320, 16, 4),
                     (130, 8, 4), (100, 12, 4), (249, 12, 3), (252, 12, 3), (253, 12, 4), (297, 16, 3), (301, 16, 4)):
        if d % (16 // np.dtype(prec).itemsize):
            continue                          # fp32 rows of 10 reals are not 16-byte pieces: below
        p = h(n, d, 64 * 512 * 2)
        assert (p["kernel"], p["rows_per_item"], p["items"], p["workgroups"]) == ("hessian_win_kl%d" % kl, 64, 1024, 512)
        assert (p["rest_items"], p["rest_workgroups"]) == (0, 0)
        # the rows behind the last whole group: a second, direct-store launch of one item
        p = h(n, d, 64 * 513 + 37)
        assert (p["kernel"], p["items"], p["workgroups"]) == ("hessian_win_kl%d" % kl, 513, 512)
        assert (p["rest_items"], p["rest_workgroups"]) == (1, 1)
        # a batch: every emulator's rest is an item of the second launch
        p = h(n, d, 1061, n_emulators=40)
        assert (p["kernel"], p["items"], p["workgroups"]) == ("hessian_win_kl%d" % kl, 640, 512)
        assert (p["rest_items"], p["rest_workgroups"]) == (40, 40)
        # fewer than 64 rows: nothing for the LDSOUT instance
        p = h(n, d, 63)
        assert (p["kernel"], p["items"], p["workgroups"], p["rest_items"]) == ("hessian_win_direct", 1, 1, 0)
        # a misaligned row or output pointer: direct stores for the whole call
        p = h(n, d, 64 * 513 + 37, aligned16=False)
        assert (p["kernel"], p["items"], p["workgroups"]) == ("hessian_win_direct", 514, 512)
        assert (p["rest_items"], p["rest_workgroups"]) == (0, 0)
    # odd kernel D, n_inputs below the kernel D: direct stores
    for n, d in ((300, 11), (250, 11), (33, 13), (250, 9), (112, 7), (64, 14), (100, 15)):
        p = h(n, d, 70000)
        assert (p["kernel"], p["rows_per_item"], p["items"], p["workgroups"]) == ("hessian_win_direct", 64, 1094, 512)
        assert (p["rest_items"], p["rest_workgroups"]) == (0, 0)
    # fp32: 16-byte pieces are 4 reals, so D = 10 stores directly; fp64: 2 reals
    p = h(250, 10, 70000)
    assert p["kernel"] == ("hessian_win_kl3" if prec == F64 else "hessian_win_direct")
    # the A/B switch sends every shape to the VALU kernel
    monkeypatch.setenv("GP_HESS_VALU", "1")
    p = h(250, 11, 70000)
    assert (p["kernel"], p["rows_per_item"], p["items"], p["workgroups"]) == ("hessian_valu", 64, 1094, 512)


def test_reconstruct_geometry_and_balanced_rounds(monkeypatch):
    monkeypatch.delenv("GP_RECON_WIDE", raising=False)
    r = lambda prec, rows, P, B, **kw: plan("reconstruct", prec, rows, n_pcs=P, n_bands=B, **kw)
    # 2101 bands: one wide workgroup covers a row in both precisions (3072 fp64 / 6144 fp32 bands)
    assert r(F64, 1000, 12, 2101) == dict(kernel="reconstruct_wide", rows_per_item=64, items=16, workgroups=16,
                                          rest_items=0, rest_workgroups=0)
    assert r(F32, 1000, 12, 2101)["kernel"] == "reconstruct_wide"
    # 4100 bands: five narrow chunks of 1024 in fp64, one wide workgroup in fp32
    p = r(F64, 1000, 5, 4100)
    assert (p["kernel"], p["items"], p["workgroups"]) == ("reconstruct_narrow", 16 * 5, 80)
    assert r(F32, 1000, 5, 4100)["kernel"] == "reconstruct_wide"
    assert r(F64, 10, 3, 1024)["kernel"] == "reconstruct_narrow" and r(F64, 10, 3, 1025)["kernel"] == "reconstruct_wide"
    assert r(F64, 10, 3, 3072)["kernel"] == "reconstruct_wide" and r(F64, 10, 3, 3073)["kernel"] == "reconstruct_narrow"
    assert r(F32, 10, 3, 2048)["kernel"] == "reconstruct_narrow" and r(F32, 10, 3, 2049)["kernel"] == "reconstruct_wide"
    assert r(F32, 10, 3, 6144)["kernel"] == "reconstruct_wide" and r(F32, 10, 3, 6145)["kernel"] == "reconstruct_narrow"
    # the cap is 4 (wide) / 8 (narrow) workgroups per compute unit; beyond it the rounds are balanced:
    # 1025 items on a cap of 1024 = two rounds of 513 and 512
    assert r(F64, 64 * 1024, 12, 2101)["workgroups"] == 1024
    p = r(F64, 64 * 1024 + 1, 12, 2101)
    assert (p["items"], p["workgroups"]) == (1025, 513)
    p = r(F64, 64 * 410, 5, 4100)                # 2050 items on a cap of 2048
    assert (p["kernel"], p["items"], p["workgroups"]) == ("reconstruct_narrow", 2050, 1025)
    p = r(F32, 64 * 2049, 12, 2101)              # three rounds of 683
    assert (p["items"], p["workgroups"]) == (2049, 683)
    monkeypatch.setenv("GP_RECON_WIDE", "0")
    assert r(F64, 1000, 12, 2101)["kernel"] == "reconstruct_narrow"
    assert (r(F64, 1000, 12, 2101)["items"], r(F64, 1000, 12, 2101)["workgroups"]) == (16 * 3, 48)
    monkeypatch.setenv("GP_RECON_WIDE", "1")
    assert r(F32, 1000, 2, 7)["kernel"] == "reconstruct_wide"


def test_workgroups_never_exceed_items_or_the_cap():
    rs = np.random.RandomState(11)
    caps = {"predict": 1, "predict_few": 10 ** 9, "generic": 4, "hessian_valu": 2, "hessian_win_kl3": 2,
            "hessian_win_kl4": 2, "hessian_win_direct": 2}
    for _ in range(400):
        op = ("predict", "mean_grad", "hessian")[rs.randint(3)]
        n, d = int(rs.randint(1, 321)), int(rs.randint(1, 17))
        E, rows, cu = int(rs.randint(1, 50)), int(rs.randint(1, 300000)), int(rs.choice([8, 64, 256, 304]))
        p = plan(op, (F64, F32)[rs.randint(2)], rows, n_train=n, n_inputs=d, n_emulators=E, cu=cu,
                 aligned16=bool(rs.randint(2)))
        assert 1 <= p["workgroups"] <= p["items"] and p["rest_workgroups"] <= p["rest_items"]
        assert p["workgroups"] <= caps[p["kernel"]] * cu or p["kernel"] == "predict_few"
        if p["kernel"].startswith("hessian_win"):
            whole = rows // 64 * E if p["kernel"] != "hessian_win_direct" else ceil_div(rows, 64) * E
            assert p["items"] == whole and p["items"] + p["rest_items"] == ceil_div(rows, 64) * E


def test_unsupported_shapes_fail_as_pack_sizes_does():
    import ctypes
    lib = _lib.load()
    for n, d in ((1100, 2), (10, 70)):
        kd, knb = ctypes.c_int(0), ctypes.c_int(0)
        rc = lib.gp_pack_sizes(_lib.GP_F64, n, d, ctypes.byref(kd), ctypes.byref(knb), None, None)
        msg = lib.gp_last_error_string()
        assert rc == -4
        for op in (_lib.GP_OP_PREDICT, _lib.GP_OP_MEAN_GRAD, _lib.GP_OP_HESSIAN):
            assert lib.gp_launch_plan(op, _lib.GP_F64, n, d, 1, 1000, 0, CU, 1, *([None] * 6)) == rc
            assert lib.gp_last_error_string() == msg
    with pytest.raises(_lib.GpuPredictError):          # as gp_hessian_device: no Hessian kernel beyond 16 inputs
        plan("hessian", F64, 100, n_train=20, n_inputs=17)
    with pytest.raises(_lib.GpuPredictError):          # as gp_predict_device: no batch on the general-shape kernel
        plan("predict", F64, 100, n_train=400, n_inputs=4, n_emulators=2)
    with pytest.raises(_lib.GpuPredictError):          # as gp_reconstruct_device
        plan("reconstruct", F64, 100, n_pcs=17, n_bands=100)
    for bad in (dict(rows=0), dict(cu=0), dict(n_emulators=0)):
        with pytest.raises(_lib.GpuPredictError):
            kw = dict(n_train=250, n_inputs=11, n_emulators=1)
            kw.update({k: v for k, v in bad.items() if k != "rows"})
            plan("predict", F64, bad.get("rows", 100), **kw)
    # every output pointer may be null
    assert lib.gp_launch_plan(_lib.GP_OP_PREDICT, _lib.GP_F64, 250, 11, 1, 1000, 0, CU, 1, *([None] * 6)) == 0

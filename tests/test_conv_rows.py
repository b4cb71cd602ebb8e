"""One-launch 1-D convolution (pow2_conv_row_kernel, kernel_pow2_conv.h): forward transform, kernel product and inverse transform of unit-stride power-of-two rows
in one kernel.  The same cases run on the CPU emulator build (unmarked) and on the device (pytest.mark.gpu).  Truth is numpy in double precision, computed as
convpad.conv_case computes it; bounds are those of the existing convolution tests (test_emu_convpad.py): relative L2 < 6e-5 in fp32, < 1e-12 in fp64."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import convpad
from helpers import Runner, rel_l2
from vkfft_amd import api

FUSED = (1, "pow2_conv_row_kernel")
# rows (C2C) / pairs of real rows (R2C) per workgroup of the registered instances, by log2 N (kernels_pow2.hip, kPow2ConvRowVariants)
FPW = {False: {6: 32, 7: 16, 8: 16, 9: 8, 10: 4, 11: 2, 12: 1, 13: 1}, True: {6: 32, 7: 16, 8: 8, 9: 4, 10: 2, 11: 1, 12: 1}}
INSTANCES = [(lg, dp) for dp in (False, True) for lg in sorted(FPW[dp])]


def bound(dp):
    return 1e-12 if dp else 6e-5


@contextlib.contextmanager
def separate_passes():
    """VKFFT_MI355X_CONV_SEPARATE=1 around plan creation: the three-launch path (the switches are read once per plan)"""
    old = os.environ.get("VKFFT_MI355X_CONV_SEPARATE")
    os.environ["VKFFT_MI355X_CONV_SEPARATE"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["VKFFT_MI355X_CONV_SEPARATE"]
        else:
            os.environ["VKFFT_MI355X_CONV_SEPARATE"] = old


def row_case(run, n, *, cf=1, nb=1, r2c=False, dp=False, conjugate=0, pad=None, separate=False, at_launch=False, seed=0):
    """1-D convolution of nb batches of cf coordinates with one kernel set of cf components.  The data buffer carries one sentinel row behind its used part, R2C rows
    carry sentinels in their two padding reals, a padded range holds NaN on entry.  Returns a dict: err (unpadded part against the truth), got, info (launch_info),
    and the hygiene flags kernel_untouched / tail_untouched / pad_reals_untouched."""
    rng = np.random.default_rng(seed)
    rt = np.float64 if dp else np.float32
    ct = np.complex128 if dp else np.complex64
    rows = nb * cf
    keep = np.ones(n, bool)
    if pad:
        keep[pad[0]:pad[1]] = False
    if r2c:
        kern = rng.uniform(-1, 1, (cf, n)).astype(rt)
        data = rng.uniform(-1, 1, (nb, cf, n)).astype(rt)
        K = np.fft.rfft(kern.astype(np.float64), axis=-1)
        X = np.fft.rfft(np.where(keep, data, 0).astype(np.float64), axis=-1)
        inv = lambda a: np.fft.irfft(a, n=n, axis=-1)
        kbuf = np.zeros((cf, n + 2), rt); kbuf[:, :n] = kern
        dbuf = np.full((rows + 1, n + 2), -77.0, rt)
        dbuf[:rows, :n] = data.reshape(rows, n)
    else:
        kern = (rng.uniform(-1, 1, (cf, n)) + 1j * rng.uniform(-1, 1, (cf, n))).astype(ct)
        data = (rng.uniform(-1, 1, (nb, cf, n)) + 1j * rng.uniform(-1, 1, (nb, cf, n))).astype(ct)
        K = np.fft.fft(kern.astype(np.complex128), axis=-1)
        X = np.fft.fft(np.where(keep, data, 0).astype(np.complex128), axis=-1)
        inv = lambda a: np.fft.ifft(a, axis=-1)
        kbuf = kern.copy()
        dbuf = np.full((rows + 1, n), -77.0 - 77.0j, ct)
        dbuf[:rows] = data.reshape(rows, n)
    if conjugate == 1:
        X = np.conj(X)
    if conjugate == 2:
        K = np.conj(K)
    want = inv(K[None] * X).reshape(rows, n)
    if pad:
        dbuf[:rows, pad[0]:pad[1]] = np.nan
    before = dbuf.copy()
    common = dict(dp=dp, r2c=r2c, lib=run.lib, normalize=True)
    hk, pk = run._alloc(kbuf)
    ka = api.App([n], 1, buffer_ptr=pk, coordinateFeatures=cf, kernelConvolution=1, **common)
    ka.forward(); ka.delete()
    kspec = run._fetch(hk, rt).copy()
    kw = dict(common, coordinateFeatures=cf, performConvolution=1, conjugateConvolution=conjugate)
    if pad:
        kw.update(performZeropadding=[1, 0, 0, 0], fft_zeropad_left=[pad[0], 0, 0, 0], fft_zeropad_right=[pad[1], 0, 0, 0])
    with (separate_passes() if separate else contextlib.nullcontext()):
        if at_launch:
            # buffer and kernel only through VkFFTLaunchParams, at non-zero byte offsets into larger allocations
            boff, koff = 4096, 2048
            hd, pd = run._alloc(np.concatenate([np.zeros(boff, np.uint8), dbuf.view(np.uint8).reshape(-1)]))
            hk2, pk2 = run._alloc(np.concatenate([np.zeros(koff, np.uint8), kspec.view(np.uint8).reshape(-1)]))
            ca = api.App([n], nb, buffer_ptr=0, specifyOffsetsAtLaunch=1, **kw)
        else:
            hd, pd = run._alloc(dbuf)
            ca = api.App([n], nb, buffer_ptr=pd, kernel=pk, **kw)
    info = ca.launch_info()
    if at_launch:
        lp = api.VkFFTLaunchParams()
        sb, sk = C.c_void_p(pd), C.c_void_p(pk2)
        lp.buffer = C.pointer(sb); lp.kernel = C.pointer(sk)
        lp.bufferOffset = boff; lp.kernelOffset = koff
        r = run.lib.VkFFTAppend(C.byref(ca.app), -1, C.byref(lp))
        assert r == 0, r
        got = run._fetch(hd, np.uint8)[boff:].copy().view(rt if r2c else ct).reshape(dbuf.shape)
        kafter = run._fetch(hk2, np.uint8)[koff:].copy().view(rt)
    else:
        ca.forward()
        got = run._fetch(hd, rt if r2c else ct).reshape(dbuf.shape)
        kafter = run._fetch(hk, rt)
    ca.delete()
    out = dict(info=info, got=got)
    res = got[:rows, :n]
    out["err"] = rel_l2(res[:, keep], want[:, keep])
    out["kernel_untouched"] = bool((kafter.reshape(-1).view(np.uint8) == kspec.reshape(-1).view(np.uint8)).all())
    out["tail_untouched"] = bool((got[rows:].view(np.uint8) == before[rows:].view(np.uint8)).all())
    if r2c:
        out["pad_reals_untouched"] = bool((got[:rows, n:] == -77.0).all())
    return out


def _batches(lg, dp, r2c, cf=2):
    """C2C: the fewest batches that give at least 3 FPW + 1 rows (three full tiles and a partial one; with cf = 2 the row count is even, so it is 3 FPW + 2
    for FPW > 1).  R2C: at least that many pairs of rows, plus one unpaired batch."""
    need = -(-(3 * FPW[dp][lg] + 1) // cf)
    return 2 * need + 1 if r2c else need


# ---- the cases: the emulator and the device run the same functions -------------------------------------------------

def check_plan_shape(run):
    for n, r2c, dp in ((1024, False, False), (256, True, True)):
        a = row_case(run, n, nb=3, r2c=r2c, dp=dp)
        assert a["info"] == FUSED, a["info"]
        assert a["err"] < bound(dp), a["err"]
        b = row_case(run, n, nb=3, r2c=r2c, dp=dp, separate=True)
        assert b["info"][0] == 3, b["info"]
        assert b["err"] < bound(dp), b["err"]
        buf = C.create_string_buffer(1024)
        # (the separate path names its product launch)
        with separate_passes():
            hk, pk = run._alloc(np.zeros(2 * (n + 2), np.float64)); hd, pd = run._alloc(np.zeros(8 * (n + 2), np.float64))
            app = api.App([n], 3, buffer_ptr=pd, kernel=pk, performConvolution=1, dp=dp, r2c=r2c, lib=run.lib)
            assert run.lib.vkfftMI355XDescribePlan(C.byref(app.app), 0, buf, 1024) == 3
            app.delete()
        assert "conv_pointwise_kernel" in buf.value.decode().split(","), buf.value


def check_instance(run, lg, dp, r2c):
    n = 1 << lg
    a = row_case(run, n, cf=2, nb=_batches(lg, dp, r2c), r2c=r2c, dp=dp, seed=lg)
    assert a["info"] == FUSED, a["info"]
    assert a["err"] < bound(dp), a["err"]
    assert a["kernel_untouched"] and a["tail_untouched"] and a.get("pad_reals_untouched", True), {k: v for k, v in a.items() if k != "got"}


def check_coordinates_that_do_not_divide_the_tile(run, n, dp, r2c):
    """(beyond the issue's list) three coordinates: the coordinate of a thread's row changes from tile to tile, the kernel spectrum is read again per tile"""
    lg = n.bit_length() - 1
    a = row_case(run, n, cf=3, nb=_batches(lg, dp, r2c, cf=3), r2c=r2c, dp=dp, seed=11)
    assert a["info"] == FUSED, a["info"]
    assert a["err"] < bound(dp), a["err"]
    assert a["kernel_untouched"] and a["tail_untouched"] and a.get("pad_reals_untouched", True)


def check_conjugation(run, dp, mode):
    a = row_case(run, 128, cf=2, nb=3, dp=dp, conjugate=mode, seed=mode)
    assert a["info"] == FUSED, a["info"]
    assert a["err"] < bound(dp), a["err"]


def check_r2c_conjugate_keeps_three_launches(run):
    for mode in (1, 2):
        err = convpad.conv_case(run, (128,), cf=2, nb=3, r2c=True, conjugate=mode, seed=mode)
        assert err < bound(False), err
        a = row_case(run, 128, cf=2, nb=3, r2c=True, conjugate=mode)
        assert a["info"][0] == 3, a["info"]
        assert a["err"] < bound(False), a["err"]


def check_zero_padding(run, n, pad, r2c, dp=False):
    a = row_case(run, n, cf=2, nb=5, r2c=r2c, dp=dp, pad=pad, seed=7)
    assert a["info"] == FUSED, a["info"]
    assert a["err"] < bound(dp), a["err"]
    # the padded range of the result is not stored: it keeps the NaN it held on entry
    assert np.isnan(a["got"][:10, pad[0]:pad[1]]).all()
    assert a["kernel_untouched"] and a["tail_untouched"] and a.get("pad_reals_untouched", True)


def check_hygiene(run, r2c, dp):
    """odd row count (an unpaired real row), a sentinel row behind the used part, sentinels in the padding reals, the kernel buffer bit by bit"""
    a = row_case(run, 256, cf=1, nb=2 * (FPW[dp][8] + 1) + 1, r2c=r2c, dp=dp, seed=3)
    assert a["info"] == FUSED, a["info"]
    assert a["err"] < bound(dp), a["err"]
    assert a["kernel_untouched"], "the kernel buffer was written"
    assert a["tail_untouched"], "a row behind the last one was written"
    if r2c:
        assert a["pad_reals_untouched"], "the padding reals of a row were written"


def check_launch_parameters(run, r2c):
    a = row_case(run, 512, cf=2, nb=5, r2c=r2c, at_launch=True, seed=9)
    assert a["info"] == FUSED, a["info"]
    assert a["err"] < bound(False), a["err"]
    assert a["kernel_untouched"] and a["tail_untouched"]


def check_plain_inverse(run):
    rng = np.random.default_rng(5)
    x = (rng.uniform(-1, 1, (3, 128)) + 1j * rng.uniform(-1, 1, (3, 128))).astype(np.complex64)
    hk, pk = run._alloc(np.ones(128, np.complex64))
    hd, pd = run._alloc(x)
    ca = api.App([128], 3, buffer_ptr=pd, performConvolution=1, kernel=pk, lib=run.lib, normalize=True)
    assert ca.launch_info() == FUSED
    ca.inverse()
    got = run._fetch(hd, np.complex64).reshape(x.shape)
    n_launch, _ = ca.launch_info(inverse=True)
    ca.delete()
    assert n_launch >= 1
    assert rel_l2(got, np.fft.ifft(x.astype(np.complex128), axis=-1)) < 2e-6


def _launches(run, shape, **kw):
    """launches of a convolution plan that is only planned (buffers of one page: never run)"""
    hk, pk = run._alloc(np.zeros(512, np.float64)); hd, pd = run._alloc(np.zeros(512, np.float64))
    app = api.App(list(shape), kw.pop("nb", 1), buffer_ptr=pd, kernel=pk, performConvolution=1, lib=run.lib, normalize=True, **kw)
    info = app.launch_info()
    app.delete()
    return info


FALLBACKS = [
    (dict(shape=(128,), m=2), dict(matrixConvolution=2, coordinateFeatures=2)),
    (dict(shape=(256,), cf=1, nk=2), dict(numberKernels=2)),
    (dict(shape=(64,), cf=2, cross=True), dict(coordinateFeatures=2, crossPowerSpectrumNormalization=1)),
    (dict(shape=(96,), cf=2, nb=2), dict(coordinateFeatures=2, nb=2)),
    (dict(shape=(1 << 15,), cf=1, nb=2), dict(nb=2)),
]


def check_fallback(run, case, plan_kw):
    c = dict(case); shape = c.pop("shape")
    err = convpad.conv_case(run, shape, **c)
    assert err < bound(False), err
    n_launch, name = _launches(run, shape, **dict(plan_kw))
    assert n_launch >= 3 and name != FUSED[1], (n_launch, name)


# ---- emulator ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def run(emu_lib):
    return Runner(emu_lib, "emu")


@pytest.fixture(scope="module")
def grun(product_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device: the library has no CPU fallback")
    return Runner(product_lib, "gpu")


ids_inst = [f"2p{lg}-{'fp64' if dp else 'fp32'}" for lg, dp in INSTANCES]
PADS = [(128, (64, 128)), (2048, (1024, 2048)), (256, (64, 160))]


def test_plan_shape(run):
    check_plan_shape(run)


@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
@pytest.mark.parametrize("lg,dp", INSTANCES, ids=ids_inst)
def test_every_instance(run, lg, dp, r2c):
    check_instance(run, lg, dp, r2c)


@pytest.mark.parametrize("n,dp,r2c", [(256, False, False), (64, True, False), (512, False, True)])
def test_three_coordinates(run, n, dp, r2c):
    check_coordinates_that_do_not_divide_the_tile(run, n, dp, r2c)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("dp", [False, True], ids=["fp32", "fp64"])
def test_conjugation(run, dp, mode):
    check_conjugation(run, dp, mode)


def test_r2c_with_conjugation_keeps_three_launches(run):
    check_r2c_conjugate_keeps_three_launches(run)


@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
@pytest.mark.parametrize("n,pad", PADS, ids=[f"{n}-{p[0]}-{p[1]}" for n, p in PADS])
def test_zero_padding(run, n, pad, r2c):
    check_zero_padding(run, n, pad, r2c, dp=(n == 256))


@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
@pytest.mark.parametrize("dp", [False, True], ids=["fp32", "fp64"])
def test_buffer_hygiene(run, r2c, dp):
    check_hygiene(run, r2c, dp)


@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
def test_launch_parameters(run, r2c):
    check_launch_parameters(run, r2c)


def test_plain_inverse_of_a_fused_application(run):
    check_plain_inverse(run)


@pytest.mark.parametrize("case,plan_kw", FALLBACKS, ids=["matrix2", "two-kernels", "cross-power", "n96", "2p15"])
def test_fallbacks_untouched(run, case, plan_kw):
    check_fallback(run, case, plan_kw)


# ---- device -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_plan_shape(grun):
    check_plan_shape(grun)


@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
@pytest.mark.parametrize("lg,dp", INSTANCES, ids=ids_inst)
def test_gpu_every_instance(grun, lg, dp, r2c):
    check_instance(grun, lg, dp, r2c)


@pytest.mark.gpu
@pytest.mark.parametrize("n,dp,r2c", [(256, False, False), (64, True, False), (512, False, True)])
def test_gpu_three_coordinates(grun, n, dp, r2c):
    check_coordinates_that_do_not_divide_the_tile(grun, n, dp, r2c)


@pytest.mark.gpu
def test_gpu_persistent_loop(grun):
    """more tiles than resident workgroups (8 per compute unit): FPW * (8 CUs + 1) rows of 64 points, about 33 MB"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = FPW[False][6] * (8 * cus + 1)
    rng = np.random.default_rng(1)
    kern = (rng.uniform(-1, 1, 64) + 1j * rng.uniform(-1, 1, 64)).astype(np.complex64)
    data = (rng.uniform(-1, 1, (rows, 64)) + 1j * rng.uniform(-1, 1, (rows, 64))).astype(np.complex64)
    want = np.fft.ifft(np.fft.fft(kern.astype(np.complex128))[None] * np.fft.fft(data.astype(np.complex128), axis=-1), axis=-1)
    hk, pk = grun._alloc(kern); hd, pd = grun._alloc(data)
    common = dict(lib=grun.lib, normalize=True)
    ka = api.App([64], 1, buffer_ptr=pk, kernelConvolution=1, **common); ka.forward(); ka.delete()
    ca = api.App([64], rows, buffer_ptr=pd, kernel=pk, performConvolution=1, **common)
    assert ca.launch_info() == FUSED
    ca.forward()
    got = grun._fetch(hd, np.complex64).reshape(data.shape)
    ca.delete()
    assert rel_l2(got, want) < bound(False)
    per_row = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    assert per_row.max() < 10 * bound(False), (int(per_row.argmax()), float(per_row.max()))  # (no tile skipped or done twice)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("dp", [False, True], ids=["fp32", "fp64"])
def test_gpu_conjugation(grun, dp, mode):
    check_conjugation(grun, dp, mode)


@pytest.mark.gpu
def test_gpu_r2c_with_conjugation_keeps_three_launches(grun):
    check_r2c_conjugate_keeps_three_launches(grun)


@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
@pytest.mark.parametrize("n,pad", PADS, ids=[f"{n}-{p[0]}-{p[1]}" for n, p in PADS])
def test_gpu_zero_padding(grun, n, pad, r2c):
    check_zero_padding(grun, n, pad, r2c, dp=(n == 256))


@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
@pytest.mark.parametrize("dp", [False, True], ids=["fp32", "fp64"])
def test_gpu_buffer_hygiene(grun, r2c, dp):
    check_hygiene(grun, r2c, dp)


@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
def test_gpu_launch_parameters(grun, r2c):
    check_launch_parameters(grun, r2c)


@pytest.mark.gpu
def test_gpu_plain_inverse_of_a_fused_application(grun):
    check_plain_inverse(grun)


@pytest.mark.gpu
@pytest.mark.parametrize("lg,dp,r2c", [(8, False, False), (12, False, True), (10, True, False)], ids=["256-fp32-c2c", "4096-fp32-r2c", "1024-fp64-c2c"])
def test_gpu_fused_agrees_with_separate_passes(grun, lg, dp, r2c):
    """both paths hold the bound against the truth, so they lie within twice the bound of each other"""
    n = 1 << lg
    kw = dict(cf=2, nb=_batches(lg, dp, r2c), r2c=r2c, dp=dp, seed=lg)
    a = row_case(grun, n, **kw)
    b = row_case(grun, n, separate=True, **kw)
    assert a["info"] == FUSED and b["info"][0] == 3, (a["info"], b["info"])
    assert a["err"] < bound(dp) and b["err"] < bound(dp), (a["err"], b["err"])
    rows = kw["nb"] * 2
    assert rel_l2(a["got"][:rows, :n], b["got"][:rows, :n]) < 2 * bound(dp)


@pytest.mark.gpu
@pytest.mark.parametrize("case,plan_kw", FALLBACKS, ids=["matrix2", "two-kernels", "cross-power", "n96", "2p15"])
def test_gpu_fallbacks_untouched(grun, case, plan_kw):
    check_fallback(grun, case, plan_kw)

"""A bank of numberKernels = K > 1 kernels on the merged last axis of a 2-D / 3-D convolution plan: mix_conv_col_bank_kernel (kernel_mix_conv_col_bank.h) on
7-smooth lengths that are no power of two, pow2_col_blue_kernel MODE 9 / 10 (kernel_pow2.h) on the non-split power-of-two lengths of 64 ... 1024 points.  The input
is transformed once, the spectrum stays in registers and product -> inverse -> store runs once per kernel: three launches instead of five for a 2-D plan.  The same
checks run on the CPU emulator build (unmarked) and on the device (pytest.mark.gpu).

Truth is numpy in double precision, ifftn(fftn(kernel_f) * fftn(x)) per kernel; bounds are those of the existing convolution tests (test_conv_rows.bound):
relative L2 < 6e-5 in fp32, < 1e-12 in fp64.  Every case draws a different random kernel per (f, v) and checks EACH result system on its own, so that a wrong
kernel offset, a wrong output slot or an input overwritten too early shows; the kernel spectra come from a kernelConvolution plan of K batches; one sentinel system
lies behind the K * cf results, and it and the kernel buffer are bit-identical afterwards.  The length lists are derived here from the rule, not read from the
generated table: a missing table entry fails.

Shapes are written as the library takes them: axis 0 (unit stride) first, the merged axis last.  Result f of coordinate v is system f * cf + v of the buffer."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from convpad import _kernel_index
from helpers import Runner, rel_l2
from test_conv_cols_mixed import SAMPLE, _chunks, _names, smooth7
from test_conv_rows import bound, separate_passes
from vkfft_amd import api

BANK = "mix_conv_col_bank_kernel"
SINGLE = "mix_conv_col_kernel"
POW2 = "pow2_col_blue_kernel"
POINTWISE = "conv_pointwise_kernel"
COLS = 37  # prime: tiles of 8 / 16 / 32 columns get four / two / one full tile and a partial one (tiles of 64: one partial tile)
# instances that are left out of the generator's table (tools/gen_mix_conv_col_bank_table.py, DROPPED): (dp, L)
DROPPED = {(False, n) for n in (576, 640, 735, 768, 810, 840, 864, 875, 882, 896, 900, 945, 960, 972, 980, 1000, 1008, 1029, 1050, 1080, 1120, 1125, 1134, 1152, 1280, 1470,
                                1536, 1568, 1575, 1620, 1680, 1715, 1728, 1764, 1792, 1800, 1875, 1890, 1920, 1944, 1960, 2000, 2016, 2025)} | {(True, n) for n in (441, 486, 490, 504)}
# the sample of the single-kernel file without the dropped lengths, and their stand-ins: every radix, every stage count, every tile width
BANK_SAMPLE = [(n, dp) for n, dp in SAMPLE if (dp, n) not in DROPPED] + [(1200, False), (1440, False), (1600, False), (1701, False), (1750, False), (480, True), (512 - 12, True)]
BANK_SAMPLE = sorted(set(BANK_SAMPLE), key=lambda e: (e[1], e[0]))
BANK_SAMPLE_IDS = [f"{n}-{'fp64' if dp else 'fp32'}" for n, dp in BANK_SAMPLE]


def lengths(dp):
    """the rule of the instance table: 7-smooth, no power of two, 12 ... 2048 (fp64: 512)"""
    return [n for n in range(12, (512 if dp else 2048) + 1) if smooth7(n) and n & (n - 1) and (dp, n) not in DROPPED]


GROUPS = [(dp, chunk) for dp in (False, True) for chunk in _chunks(lengths(dp), 40)]
GROUP_IDS = [f"{'fp64' if dp else 'fp32'}-{chunk[0]}-{chunk[-1]}" for dp, chunk in GROUPS]


def test_the_rule_gives_the_documented_instance_counts():
    assert [len(lengths(dp)) for dp in (False, True)] == [172 - 44, 90 - 4]
    assert [len(lengths(dp)) + sum(1 for d, _ in DROPPED if d == dp) for dp in (False, True)] == [172, 90]
    assert all((dp, n) not in DROPPED for n, dp in BANK_SAMPLE)


def bank_case(run, shape, nk, *, cf=1, m=1, symmetric=False, r2c=False, dp=False, conjugate=0, cross=False, pads=None, separate=False, at_launch=False, seed=0):
    """One input of cf coordinates (m > 1: matrixConvolution = m, cf = m) against nk kernels.  The buffer holds nk * cf result systems and one sentinel system; the
    input lies in the first cf, the others hold 55 on entry; every padded range holds NaN on entry, in all nk * cf systems.  Returns a dict: names (launches, kernel
    names), got, errs (one relative error per result system, unpadded part against the truth), err (all of them together) and the hygiene flags kernel_untouched /
    tail_untouched / padded_still_nan (the padded range of the last axis of all nk * cf systems)."""
    rng = np.random.default_rng(seed)
    rt = np.float64 if dp else np.float32
    ct = np.complex128 if dp else np.complex64
    dims = tuple(reversed(shape)); nd = len(dims); ax = tuple(range(-nd, 0))
    if m > 1:
        cf = m
    ksys = (m * (m + 1) // 2 if symmetric else m * m) if m > 1 else cf
    nres = nk * cf
    keep = np.ones(dims, bool)
    left = [0] * 4; right = [0] * 4; flag = [0] * 4
    for a, (l, r) in (pads or {}).items():
        left[a], right[a], flag[a] = l, r, 1
        idx = [slice(None)] * nd; idx[nd - 1 - a] = slice(l, r); keep[tuple(idx)] = False
    nx = shape[0]
    if r2c:
        pitch = dims[:-1] + (nx + 2,)
        kern = rng.uniform(-1, 1, (nk, ksys) + dims).astype(rt)
        data = rng.uniform(-1, 1, (cf,) + dims).astype(rt)
        fwd = lambda a: np.fft.rfftn(a.astype(np.float64), axes=ax)
        inv = lambda a: np.fft.irfftn(a, s=dims, axes=ax)
        kbuf = np.zeros((nk, ksys) + pitch, rt); kbuf[..., :nx] = kern
        dbuf = np.full((nres + 1,) + pitch, -77.0, rt)
        dbuf[:nres, ..., :nx] = np.where(keep, rt(55.0), rt(np.nan))
        dbuf[:cf, ..., :nx] = np.where(keep, data, np.nan)
    else:
        kern = (rng.uniform(-1, 1, (nk, ksys) + dims) + 1j * rng.uniform(-1, 1, (nk, ksys) + dims)).astype(ct)
        data = (rng.uniform(-1, 1, (cf,) + dims) + 1j * rng.uniform(-1, 1, (cf,) + dims)).astype(ct)
        fwd = lambda a: np.fft.fftn(a.astype(np.complex128), axes=ax)
        inv = lambda a: np.fft.ifftn(a, axes=ax)
        kbuf = kern.copy()
        dbuf = np.full((nres + 1,) + dims, -77.0 - 77.0j, ct)
        dbuf[:nres] = np.where(keep, ct(55.0 + 55.0j), ct(np.nan + 1j * np.nan))
        dbuf[:cf] = np.where(keep, data, np.nan + 1j * np.nan)
    K, X = fwd(kern), fwd(np.where(keep, data, 0))
    if conjugate == 1:
        X = np.conj(X)
    if conjugate == 2:
        K = np.conj(K)
    Y = np.zeros((nk, cf) + X.shape[1:], np.complex128)
    for f in range(nk):
        if m > 1:
            for j in range(m):
                for l in range(m):
                    Y[f, j] += K[f, _kernel_index(j, l, m, symmetric)] * X[l]
        else:
            Y[f] = K[f] * X
    if cross:
        Y = Y / np.abs(Y)
    want = inv(Y).reshape((nres,) + dims)
    before = dbuf.copy()
    common = dict(dp=dp, r2c=r2c, lib=run.lib, normalize=True)
    hk, pk = run._alloc(kbuf)
    ka = api.App(list(shape), nk, buffer_ptr=pk, coordinateFeatures=ksys, kernelConvolution=1, **common)
    ka.forward(); ka.delete()
    kspec = run._fetch(hk, rt).copy()
    kw = dict(common, coordinateFeatures=cf, performConvolution=1, numberKernels=nk, matrixConvolution=m, symmetricKernel=int(symmetric), conjugateConvolution=conjugate,
              crossPowerSpectrumNormalization=int(cross))
    if pads:
        kw.update(performZeropadding=flag, fft_zeropad_left=left, fft_zeropad_right=right)
    with (separate_passes() if separate else contextlib.nullcontext()):
        if at_launch:
            # buffer and kernel only through VkFFTLaunchParams, at non-zero byte offsets into larger allocations
            boff, koff = 4096, 2048
            hd, pd = run._alloc(np.concatenate([np.zeros(boff, np.uint8), dbuf.view(np.uint8).reshape(-1)]))
            hk2, pk2 = run._alloc(np.concatenate([np.zeros(koff, np.uint8), kspec.view(np.uint8).reshape(-1)]))
            ca = api.App(list(shape), 1, buffer_ptr=0, specifyOffsetsAtLaunch=1, **kw)
        else:
            hd, pd = run._alloc(dbuf)
            ca = api.App(list(shape), 1, buffer_ptr=pd, kernel=pk, **kw)
    names = _names(ca)
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
    res = got[:nres, ..., :nx]
    out = dict(names=names, got=res)
    out["errs"] = [rel_l2(res[s][keep], want[s][keep]) for s in range(nres)]
    out["err"] = rel_l2(res[:, keep], want[:, keep])
    out["kernel_untouched"] = bool((kafter.reshape(-1).view(np.uint8) == kspec.reshape(-1).view(np.uint8)).all())
    out["tail_untouched"] = bool((got[nres:].view(np.uint8) == before[nres:].view(np.uint8)).all())
    last = nd - 1
    if pads and last in pads:
        idx = [slice(None)] * (nd + 1); idx[1] = slice(*pads[last])
        out["padded_still_nan"] = bool(np.isnan(res[tuple(idx)]).all())
    return out


def assert_good(a, dp, tag=None):
    """each result system on its own, the sentinel system and the kernel buffer"""
    print(f"{tag}: worst system rel L2 {max(a['errs']):.3e}")
    assert max(a["errs"]) < bound(dp), (tag, a["errs"])
    assert a["kernel_untouched"], (tag, "the kernel buffer was written")
    assert a["tail_untouched"], (tag, "the system behind the last result was written")


def bank_merged(a):
    launches, names = a["names"]
    return BANK in names and POINTWISE not in names and SINGLE not in names


def pow2_merged(a):
    launches, names = a["names"]
    return POW2 in names and POINTWISE not in names


# ---- the checks: the emulator and the device run the same functions ------------------------------------------------

PLAN_SHAPES = [((16, 360), False, False, 3, BANK), ((16, 100), True, True, 2, BANK), ((16, 256), False, False, 3, POW2)]
PLAN_IDS = ["16x360-fp32-K3", "r2c-16x100-fp64-K2", "16x256-fp32-K3"]


def check_plan_shape(run, shape, r2c, dp, nk, kernel):
    a = bank_case(run, shape, nk, r2c=r2c, dp=dp)
    launches, names = a["names"]
    assert launches == 3 and kernel in names and POINTWISE not in names, a["names"]
    assert_good(a, dp, shape)
    b = bank_case(run, shape, nk, r2c=r2c, dp=dp, separate=True)
    launches, names = b["names"]
    assert launches == 5 and POINTWISE in names and BANK not in names, b["names"]
    assert_good(b, dp, shape)
    assert rel_l2(a["got"], b["got"]) < 2 * bound(dp)


def check_instance(run, n, dp):
    a = bank_case(run, (COLS, n), 2, dp=dp, seed=n)
    tag = (n, dp)
    assert bank_merged(a) and a["names"][0] == 3, (tag, a["names"])
    assert_good(a, dp, tag)


POW2_CASES = [((16, 64), dict(nk=3)), ((16, 256), dict(nk=3)), ((16, 1024), dict(nk=3)), ((16, 128), dict(nk=2, m=2)), ((16, 512), dict(nk=3, m=3, symmetric=True)),
              ((16, 1024), dict(nk=2, m=2)), ((16, 256), dict(nk=2, m=2, dp=True))]
POW2_IDS = ["16x64-K3", "16x256-K3", "16x1024-K3", "16x128-matrix2-K2", "16x512-matrix3-symmetric-K3", "16x1024-matrix2-K2-narrow", "fp64-16x256-matrix2-K2"]


def check_pow2(run, shape, kw):
    kw = dict(kw); nk = kw.pop("nk")
    a = bank_case(run, shape, nk, seed=shape[1] + nk, **kw)
    assert pow2_merged(a) and a["names"][0] == 3, a["names"]
    assert_good(a, kw.get("dp", False), (shape, kw))


def check_coordinates(run, cf, dp):
    a = bank_case(run, (16, 360), 3, cf=cf, dp=dp, seed=11 + cf)
    assert bank_merged(a) and a["names"][0] == 3, a["names"]
    assert_good(a, dp, cf)


def check_conjugation(run, mode, r2c):
    a = bank_case(run, (16, 120), 2, cf=2, r2c=r2c, conjugate=mode, seed=mode)
    assert bank_merged(a), a["names"]
    assert_good(a, False, mode)


VOLUMES = [((8, 6, 360), False), ((10, 5, 120), True)]
VOLUME_IDS = ["8x6x360", "r2c-10x5x120"]
WIDTHS = [(1, 120), (32, 100)]
WIDTH_IDS = ["1x120", "32x100"]


def check_shape(run, shape, r2c):
    a = bank_case(run, shape, 2, r2c=r2c, seed=4)
    assert bank_merged(a), a["names"]
    assert_good(a, False, shape)


def check_launch_parameters(run):
    a = bank_case(run, (20, 600), 3, cf=2, at_launch=True, seed=9)
    assert bank_merged(a), a["names"]
    assert_good(a, False)


def check_plain_inverse(run):
    """VkFFTAppend(app, 1) of a bank application: the plain inverse of all K systems over every axis"""
    rng = np.random.default_rng(5)
    x = (rng.uniform(-1, 1, (3, 120, 16)) + 1j * rng.uniform(-1, 1, (3, 120, 16))).astype(np.complex64)
    hk, pk = run._alloc(np.ones((3, 120, 16), np.complex64))
    hd, pd = run._alloc(x)
    ca = api.App([16, 120], 1, buffer_ptr=pd, performConvolution=1, numberKernels=3, kernel=pk, lib=run.lib, normalize=True)
    assert BANK in _names(ca)[1]
    ca.inverse()
    got = run._fetch(hd, np.complex64).reshape(x.shape)
    n_launch, names = _names(ca, inverse=True)
    ca.delete()
    assert n_launch >= 1 and BANK not in names, (n_launch, names)
    assert rel_l2(got, np.fft.ifftn(x.astype(np.complex128), axes=(-2, -1))) < 2e-6


PADS = [((16, 360), {1: (180, 360)}), ((32, 360), {0: (16, 32), 1: (180, 360)})]
PAD_IDS = ["16x360-180-360", "32x360-both-axes"]


def check_zero_padding(run, shape, pads):
    a = bank_case(run, shape, 3, cf=2, pads=pads, seed=7)
    assert bank_merged(a), a["names"]
    # the padded range is neither read (the results would be NaN) nor written, in any of the K results: it keeps the NaN it held on entry
    assert a["padded_still_nan"]
    assert_good(a, False, shape)


FALLBACKS = [
    ("16x2048-split-form", (16, 2048), dict()),
    ("16x360-matrix2", (16, 360), dict(m=2)),
    ("16x390-factor-13", (16, 390), dict()),
    ("16x1080-dropped-length", (16, 1080), dict()),
    ("cross-power", (16, 360), dict(cf=2, cross=True)),
    ("separate-switch", (16, 360), dict(separate=True)),
]
FALLBACK_IDS = [f[0] for f in FALLBACKS]


def check_fallback(run, shape, kw):
    a = bank_case(run, shape, 2, seed=13, **kw)
    launches, names = a["names"]
    assert launches >= 5 and POINTWISE in names and BANK not in names, a["names"]
    assert_good(a, False, (shape, kw))


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


@pytest.mark.parametrize("shape,r2c,dp,nk,kernel", PLAN_SHAPES, ids=PLAN_IDS)
def test_plan_shape(run, shape, r2c, dp, nk, kernel):
    check_plan_shape(run, shape, r2c, dp, nk, kernel)


@pytest.mark.parametrize("n,dp", BANK_SAMPLE, ids=BANK_SAMPLE_IDS)
def test_every_instance_class(run, n, dp):
    check_instance(run, n, dp)


@pytest.mark.parametrize("shape,kw", POW2_CASES, ids=POW2_IDS)
def test_power_of_two(run, shape, kw):
    check_pow2(run, shape, kw)


@pytest.mark.parametrize("cf", [2, 3])
@pytest.mark.parametrize("dp", [False, True], ids=["fp32", "fp64"])
def test_coordinates(run, dp, cf):
    check_coordinates(run, cf, dp)


@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
@pytest.mark.parametrize("mode", [1, 2])
def test_conjugation(run, mode, r2c):
    check_conjugation(run, mode, r2c)


@pytest.mark.parametrize("shape,r2c", VOLUMES, ids=VOLUME_IDS)
def test_three_dimensions(run, shape, r2c):
    check_shape(run, shape, r2c)


@pytest.mark.parametrize("shape", WIDTHS, ids=WIDTH_IDS)
def test_narrow_and_exact_widths(run, shape):
    check_shape(run, shape, False)


def test_launch_parameters(run):
    check_launch_parameters(run)


def test_plain_inverse_of_a_bank_application(run):
    check_plain_inverse(run)


@pytest.mark.parametrize("shape,pads", PADS, ids=PAD_IDS)
def test_zero_padding(run, shape, pads):
    check_zero_padding(run, shape, pads)


@pytest.mark.parametrize("name,shape,kw", FALLBACKS, ids=FALLBACK_IDS)
def test_fallbacks_keep_the_separate_passes(run, name, shape, kw):
    check_fallback(run, shape, kw)


# ---- device -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape,r2c,dp,nk,kernel", PLAN_SHAPES, ids=PLAN_IDS)
def test_gpu_plan_shape(grun, shape, r2c, dp, nk, kernel):
    check_plan_shape(grun, shape, r2c, dp, nk, kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("dp,group", GROUPS, ids=GROUP_IDS)
def test_gpu_every_instance(grun, dp, group):
    for n in group:
        check_instance(grun, n, dp)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kw", POW2_CASES, ids=POW2_IDS)
def test_gpu_power_of_two(grun, shape, kw):
    check_pow2(grun, shape, kw)


@pytest.mark.gpu
@pytest.mark.parametrize("cf", [2, 3])
@pytest.mark.parametrize("dp", [False, True], ids=["fp32", "fp64"])
def test_gpu_coordinates(grun, dp, cf):
    check_coordinates(grun, cf, dp)


@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
@pytest.mark.parametrize("mode", [1, 2])
def test_gpu_conjugation(grun, mode, r2c):
    check_conjugation(grun, mode, r2c)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,r2c", VOLUMES, ids=VOLUME_IDS)
def test_gpu_three_dimensions(grun, shape, r2c):
    check_shape(grun, shape, r2c)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", WIDTHS, ids=WIDTH_IDS)
def test_gpu_narrow_and_exact_widths(grun, shape):
    check_shape(grun, shape, False)


@pytest.mark.gpu
def test_gpu_launch_parameters(grun):
    check_launch_parameters(grun)


@pytest.mark.gpu
def test_gpu_plain_inverse_of_a_bank_application(grun):
    check_plain_inverse(grun)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,pads", PADS, ids=PAD_IDS)
def test_gpu_zero_padding(grun, shape, pads):
    check_zero_padding(grun, shape, pads)


@pytest.mark.gpu
@pytest.mark.parametrize("name,shape,kw", FALLBACKS, ids=FALLBACK_IDS)
def test_gpu_fallbacks_keep_the_separate_passes(grun, name, shape, kw):
    check_fallback(grun, shape, kw)

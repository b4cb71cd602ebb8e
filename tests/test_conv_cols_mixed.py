"""Merged last axis of a 2-D / 3-D convolution plan on 7-smooth lengths that are no power of two (mix_conv_col_kernel, kernel_mix_conv_col.h): last axis forward,
kernel product and last axis backwards of a strided axis of 12 ... 2048 points (fp64: ... 512) in one kernel, three launches instead of five for a 2-D plan.  The
same checks run on the CPU emulator build (unmarked) and on the device (pytest.mark.gpu).  Truth is numpy in double precision (plane_case, built like
test_conv_rows.row_case); bounds are those of the existing convolution tests: relative L2 < 6e-5 in fp32, < 1e-12 in fp64.  The length lists are derived here from
the rule, not read from the generated table: a missing table entry fails.

Shapes are written as the library takes them: axis 0 (unit stride) first, the merged axis last.

(The two padding reals of a row of an R2C plan are NOT checked here, other than in the 1-D row tests: the in-place R2C pass along axis 0 keeps the Nyquist bin in
them, on the separate passes and in the reference alike; the merged kernel transforms that bin as one more column.  The sentinel system behind the data and the
kernel buffer are checked in every case.)"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import convpad
from helpers import Runner, rel_l2
from test_conv_rows import bound, separate_passes
from vkfft_amd import api

KERNEL = "mix_conv_col_kernel"
POINTWISE = "conv_pointwise_kernel"
COLS = 37  # prime: tiles of 8 / 16 / 32 columns get four / two / one full tile and a partial one (tiles of 64: one partial tile)
# instances that are left out of the generator's table (tools/gen_mix_conv_col_table.py, DROPPED): (dp, L)
DROPPED = set()


def smooth7(n):
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def lengths(dp):
    """the rule of the instance table: 7-smooth, no power of two, 12 ... 2048 (fp64: 512)"""
    return [n for n in range(12, (512 if dp else 2048) + 1) if smooth7(n) and n & (n - 1) and (dp, n) not in DROPPED]


def _chunks(seq, size):
    return [seq[i:i + size] for i in range(0, len(seq), size)]


GROUPS = [(dp, chunk) for dp in (False, True) for chunk in _chunks(lengths(dp), 40)]
GROUP_IDS = [f"{'fp64' if dp else 'fp32'}-{chunk[0]}-{chunk[-1]}" for dp, chunk in GROUPS]

# every radix, every stage count, every tile width
SAMPLE = [(n, False) for n in (12, 24, 60, 96, 100, 120, 243, 343, 360, 625, 1000, 1080, 1536, 1920, 2000, 2025)] + [(n, True) for n in (12, 100, 243, 360, 500, 504)]
SAMPLE_IDS = [f"{n}-{'fp64' if dp else 'fp32'}" for n, dp in SAMPLE]


def test_the_rule_gives_the_documented_instance_counts():
    assert DROPPED == set()
    assert [len(lengths(dp)) + sum(1 for d, _ in DROPPED if d == dp) for dp in (False, True)] == [172, 90]
    assert all(len(g[1]) <= 40 for g in GROUPS)


def _names(app, inverse=False):
    buf = C.create_string_buffer(2048)
    n = app.lib.vkfftMI355XDescribePlan(C.byref(app.app), 1 if inverse else 0, buf, 2048)
    return int(n), [x.split("<")[0] for x in buf.value.decode().split(",") if x]


def plan_names(run, shape, nb=1, **kw):
    """(launches, names) of a convolution plan that is only planned (buffers of one page: never run)"""
    hk, pk = run._alloc(np.zeros(512, np.float64)); hd, pd = run._alloc(np.zeros(512, np.float64))
    app = api.App(list(shape), nb, buffer_ptr=pd, kernel=pk, performConvolution=1, lib=run.lib, normalize=True, **kw)
    out = _names(app)
    app.delete()
    return out


def plane_case(run, shape, *, cf=1, nb=1, r2c=False, dp=False, conjugate=0, pads=None, separate=False, at_launch=False, seed=0):
    """Convolution of nb batches of cf coordinates with one kernel set of cf components (a random kernel per coordinate).  The data buffer carries one sentinel
    system behind its used part; every padded range holds NaN on entry (padded_still_nan: the padded range of the last axis still does afterwards).  Returns a dict: err (unpadded part against the truth), got (the systems, without the
    padding reals of an R2C plan), names (launches, kernel names), worst_system (the largest error of one system), and the hygiene flags kernel_untouched / tail_untouched / padded_still_nan."""
    rng = np.random.default_rng(seed)
    rt = np.float64 if dp else np.float32
    ct = np.complex128 if dp else np.complex64
    dims = tuple(reversed(shape)); nd = len(dims); ax = tuple(range(-nd, 0))
    nsys = nb * cf
    keep = np.ones(dims, bool)
    left = [0] * 4; right = [0] * 4; flag = [0] * 4
    for a, (l, r) in (pads or {}).items():
        left[a], right[a], flag[a] = l, r, 1
        idx = [slice(None)] * nd; idx[nd - 1 - a] = slice(l, r); keep[tuple(idx)] = False
    if r2c:
        nx = shape[0]; pitch = dims[:-1] + (nx + 2,)
        kern = rng.uniform(-1, 1, (cf,) + dims).astype(rt)
        data = rng.uniform(-1, 1, (nb, cf) + dims).astype(rt)
        fwd = lambda a: np.fft.rfftn(a.astype(np.float64), axes=ax)
        inv = lambda a: np.fft.irfftn(a, s=dims, axes=ax)
        kbuf = np.zeros((cf,) + pitch, rt); kbuf[..., :nx] = kern
        dbuf = np.full((nsys + 1,) + pitch, -77.0, rt)
        dbuf[:nsys, ..., :nx] = np.where(keep, data, np.nan).reshape((nsys,) + dims)
    else:
        nx = shape[0]
        kern = (rng.uniform(-1, 1, (cf,) + dims) + 1j * rng.uniform(-1, 1, (cf,) + dims)).astype(ct)
        data = (rng.uniform(-1, 1, (nb, cf) + dims) + 1j * rng.uniform(-1, 1, (nb, cf) + dims)).astype(ct)
        fwd = lambda a: np.fft.fftn(a.astype(np.complex128), axes=ax)
        inv = lambda a: np.fft.ifftn(a, axes=ax)
        kbuf = kern.copy()
        dbuf = np.full((nsys + 1,) + dims, -77.0 - 77.0j, ct)
        dbuf[:nsys] = np.where(keep, data, np.nan + 1j * np.nan).reshape((nsys,) + dims)
    K, X = fwd(kern), fwd(np.where(keep, data, 0))
    if conjugate == 1:
        X = np.conj(X)
    if conjugate == 2:
        K = np.conj(K)
    want = inv(K[None] * X).reshape((nsys,) + dims)
    before = dbuf.copy()
    common = dict(dp=dp, r2c=r2c, lib=run.lib, normalize=True)
    hk, pk = run._alloc(kbuf)
    ka = api.App(list(shape), 1, buffer_ptr=pk, coordinateFeatures=cf, kernelConvolution=1, **common)
    ka.forward(); ka.delete()
    kspec = run._fetch(hk, rt).copy()
    kw = dict(common, coordinateFeatures=cf, performConvolution=1, conjugateConvolution=conjugate)
    if pads:
        kw.update(performZeropadding=flag, fft_zeropad_left=left, fft_zeropad_right=right)
    with (separate_passes() if separate else contextlib.nullcontext()):
        if at_launch:
            # buffer and kernel only through VkFFTLaunchParams, at non-zero byte offsets into larger allocations
            boff, koff = 4096, 2048
            hd, pd = run._alloc(np.concatenate([np.zeros(boff, np.uint8), dbuf.view(np.uint8).reshape(-1)]))
            hk2, pk2 = run._alloc(np.concatenate([np.zeros(koff, np.uint8), kspec.view(np.uint8).reshape(-1)]))
            ca = api.App(list(shape), nb, buffer_ptr=0, specifyOffsetsAtLaunch=1, **kw)
        else:
            hd, pd = run._alloc(dbuf)
            ca = api.App(list(shape), nb, buffer_ptr=pd, kernel=pk, **kw)
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
    res = got[:nsys, ..., :nx]
    out = dict(names=names, got=res)
    out["err"] = rel_l2(res[:, keep], want[:, keep])
    out["worst_system"] = max(rel_l2(res[s][keep], want[s][keep]) for s in range(nsys))
    out["kernel_untouched"] = bool((kafter.reshape(-1).view(np.uint8) == kspec.reshape(-1).view(np.uint8)).all())
    out["tail_untouched"] = bool((got[nsys:].view(np.uint8) == before[nsys:].view(np.uint8)).all())
    # the padded range of the LAST axis (rows that no pass visits; the padded range of axis 0 holds the spectrum between the passes, on every path)
    last = nd - 1
    if pads and last in pads:
        idx = [slice(None)] * (nd + 1); idx[1] = slice(*pads[last])
        out["padded_still_nan"] = bool(np.isnan(res[tuple(idx)]).all())
    return out


def merged(a):
    launches, names = a["names"]
    return KERNEL in names and POINTWISE not in names


def assert_clean(a, tag=None):
    assert a["kernel_untouched"], (tag, "the kernel buffer was written")
    assert a["tail_untouched"], (tag, "the system behind the last one was written")


# ---- the checks: the emulator and the device run the same functions ------------------------------------------------

def check_plan_shape(run):
    for shape, r2c, dp, nb in (((16, 360), False, False, 2), ((16, 100), True, True, 1)):
        a = plane_case(run, shape, nb=nb, r2c=r2c, dp=dp)
        launches, names = a["names"]
        assert launches == 3 and KERNEL in names and POINTWISE not in names, a["names"]
        assert a["err"] < bound(dp), a["err"]
        b = plane_case(run, shape, nb=nb, r2c=r2c, dp=dp, separate=True)
        launches, names = b["names"]
        assert launches == 5 and POINTWISE in names and KERNEL not in names, b["names"]
        assert b["err"] < bound(dp), b["err"]
        assert rel_l2(a["got"], b["got"]) < 2 * bound(dp)
        with separate_passes():
            launches, names = plan_names(run, shape, nb=nb, dp=dp, r2c=r2c)
        assert launches == 5 and POINTWISE in names and KERNEL not in names, (launches, names)


def check_instance(run, n, dp):
    a = plane_case(run, (COLS, n), nb=2, dp=dp, seed=n)
    tag = (n, dp)
    assert merged(a) and a["names"][0] == 3, (tag, a["names"])
    print(f"L={n} {'fp64' if dp else 'fp32'}: rel L2 {a['err']:.3e}")
    assert a["err"] < bound(dp), (tag, a["err"])
    assert_clean(a, tag)


def check_width(run, shape, r2c):
    a = plane_case(run, shape, nb=2, r2c=r2c, seed=3)
    assert merged(a), a["names"]
    assert a["err"] < bound(False), a["err"]
    assert_clean(a, shape)


def check_volume(run, shape, nb, r2c):
    a = plane_case(run, shape, nb=nb, r2c=r2c, seed=4)
    assert merged(a), a["names"]
    assert a["err"] < bound(False), a["err"]
    assert_clean(a, shape)


def check_coordinates(run, cf, dp):
    """a random kernel per coordinate: a wrong kernel offset shows"""
    a = plane_case(run, (16, 360), cf=cf, nb=5, dp=dp, seed=11 + cf)
    assert merged(a) and a["names"][0] == 3, a["names"]
    assert a["err"] < bound(dp), a["err"]
    assert a["worst_system"] < bound(dp), a["worst_system"]
    assert_clean(a, cf)


def check_conjugation(run, mode, r2c, dp):
    a = plane_case(run, (16, 120), cf=2, nb=3, r2c=r2c, dp=dp, conjugate=mode, seed=mode)
    assert merged(a), a["names"]
    assert a["err"] < bound(dp), a["err"]
    assert_clean(a, mode)


def check_zero_padding(run, shape, pads, r2c, dp):
    a = plane_case(run, shape, cf=2, nb=2, r2c=r2c, dp=dp, pads=pads, seed=7)
    assert merged(a), a["names"]
    assert a["err"] < bound(dp), a["err"]
    # the padded range is neither read (the result would be NaN) nor written: it keeps the NaN it held on entry
    assert a["padded_still_nan"]
    assert_clean(a, shape)


def check_launch_parameters(run, r2c):
    a = plane_case(run, (20, 600), cf=2, nb=3, r2c=r2c, at_launch=True, seed=9)
    assert merged(a), a["names"]
    assert a["err"] < bound(False), a["err"]
    assert_clean(a)


def check_plain_inverse(run):
    rng = np.random.default_rng(5)
    x = (rng.uniform(-1, 1, (3, 120, 16)) + 1j * rng.uniform(-1, 1, (3, 120, 16))).astype(np.complex64)
    hk, pk = run._alloc(np.ones((120, 16), np.complex64))
    hd, pd = run._alloc(x)
    ca = api.App([16, 120], 3, buffer_ptr=pd, performConvolution=1, kernel=pk, lib=run.lib, normalize=True)
    assert KERNEL in _names(ca)[1]
    ca.inverse()
    got = run._fetch(hd, np.complex64).reshape(x.shape)
    n_launch, names = _names(ca, inverse=True)
    ca.delete()
    assert n_launch >= 1 and KERNEL not in names, (n_launch, names)
    assert rel_l2(got, np.fft.ifftn(x.astype(np.complex128), axes=(-2, -1))) < 2e-6


def _special_fallback(run, which):
    """frequencyZeroPadding / a separate input buffer on (16, 360): conv_case has neither.  Returns (err, launches, names)"""
    rng = np.random.default_rng(21)
    dims = (360, 16)
    kern = (rng.uniform(-1, 1, dims) + 1j * rng.uniform(-1, 1, dims)).astype(np.complex64)
    data = (rng.uniform(-1, 1, (2,) + dims) + 1j * rng.uniform(-1, 1, (2,) + dims)).astype(np.complex64)
    Y = np.fft.fft2(kern.astype(np.complex128))[None] * np.fft.fft2(data.astype(np.complex128))
    kw = dict(lib=run.lib, normalize=True)
    hk, pk = run._alloc(kern)
    ka = api.App([16, 360], 1, buffer_ptr=pk, kernelConvolution=1, **kw); ka.forward(); ka.delete()
    if which == "frequency":
        # the range [90, 200) of the last axis of the product's spectrum is taken as zero by the inverse half
        Y[:, 90:200, :] = 0
        hd, pd = run._alloc(data)
        ca = api.App([16, 360], 2, buffer_ptr=pd, kernel=pk, performConvolution=1, performZeropadding=[0, 1, 0, 0], fft_zeropad_left=[0, 90, 0, 0],
                     fft_zeropad_right=[0, 200, 0, 0], frequencyZeroPadding=1, **kw)
    else:
        hin, pin = run._alloc(data)
        hd, pd = run._alloc(np.zeros_like(data))
        ca = api.App([16, 360], 2, buffer_ptr=pd, kernel=pk, performConvolution=1, isInputFormatted=1, inputBuffer=pin, **kw)
    launches, names = _names(ca)
    ca.forward()
    got = run._fetch(hd, np.complex64).reshape(data.shape)
    ca.delete()
    return rel_l2(got, np.fft.ifft2(Y)), launches, names


# (what conv_case runs, what the plan is created with, double precision)
FALLBACKS = [
    ("16x390-factor-13", dict(shape=(16, 390), nb=2), dict(nb=2), False),
    ("16x2100-above-the-range", dict(shape=(16, 2100), nb=2), dict(nb=2), False),
    ("fp64-16x525", dict(shape=(16, 525), nb=2, dp=True), dict(nb=2, dp=True), True),
    ("matrix2", dict(shape=(16, 360), m=2), dict(matrixConvolution=2, coordinateFeatures=2), False),
    ("two-kernels", dict(shape=(16, 360), nk=2), dict(numberKernels=2), False),
    ("cross-power", dict(shape=(16, 360), cf=2, cross=True), dict(coordinateFeatures=2, crossPowerSpectrumNormalization=1), False),
    ("16x6-below-the-floor", dict(shape=(16, 6), nb=2), dict(nb=2), False),
]
FALLBACK_IDS = [f[0] for f in FALLBACKS]


def check_fallback(run, case, plan_kw, dp):
    c = dict(case); shape = c.pop("shape")
    err = convpad.conv_case(run, shape, **c)
    assert err < bound(dp), err
    launches, names = plan_names(run, shape, **dict(plan_kw))
    assert launches >= 3 and KERNEL not in names, (launches, names)


def check_special_fallback(run, which):
    err, launches, names = _special_fallback(run, which)
    assert err < bound(False), err
    assert launches >= 3 and KERNEL not in names, (launches, names)


WIDTHS = [((2, 360), True), ((1, 120), False), ((32, 100), False)]
WIDTH_IDS = ["r2c-2x360", "1x120", "32x100"]
VOLUMES = [((8, 6, 360), 3, False), ((10, 5, 120), 1, True)]
VOLUME_IDS = ["8x6x360-nb3", "r2c-10x5x120"]
CONJ = [(mode, r2c, dp) for mode in (1, 2) for r2c in (False, True) for dp in (False, True)]
CONJ_IDS = [f"mode{m}-{'r2c' if r else 'c2c'}-{'fp64' if d else 'fp32'}" for m, r, d in CONJ]
PADS = [((16, 360), {1: (180, 360)}, False, False), ((16, 360), {1: (90, 200)}, False, True), ((32, 360), {0: (16, 32), 1: (180, 360)}, False, False),
        ((32, 360), {0: (16, 32), 1: (180, 360)}, True, False)]
PAD_IDS = ["16x360-180-360", "fp64-16x360-90-200", "32x360-both-axes", "r2c-32x360-both-axes"]


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


def test_plan_shape(run):
    check_plan_shape(run)


@pytest.mark.parametrize("n,dp", SAMPLE, ids=SAMPLE_IDS)
def test_every_instance_class(run, n, dp):
    check_instance(run, n, dp)


@pytest.mark.parametrize("shape,r2c", WIDTHS, ids=WIDTH_IDS)
def test_narrow_and_exact_widths(run, shape, r2c):
    check_width(run, shape, r2c)


@pytest.mark.parametrize("shape,nb,r2c", VOLUMES, ids=VOLUME_IDS)
def test_three_dimensions(run, shape, nb, r2c):
    check_volume(run, shape, nb, r2c)


@pytest.mark.parametrize("cf", [2, 3])
@pytest.mark.parametrize("dp", [False, True], ids=["fp32", "fp64"])
def test_coordinates(run, dp, cf):
    check_coordinates(run, cf, dp)


@pytest.mark.parametrize("mode,r2c,dp", CONJ, ids=CONJ_IDS)
def test_conjugation(run, mode, r2c, dp):
    check_conjugation(run, mode, r2c, dp)


@pytest.mark.parametrize("shape,pads,r2c,dp", PADS, ids=PAD_IDS)
def test_zero_padding(run, shape, pads, r2c, dp):
    check_zero_padding(run, shape, pads, r2c, dp)


@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
def test_launch_parameters(run, r2c):
    check_launch_parameters(run, r2c)


def test_plain_inverse_of_a_merged_application(run):
    check_plain_inverse(run)


@pytest.mark.parametrize("name,case,plan_kw,dp", FALLBACKS, ids=FALLBACK_IDS)
def test_fallbacks_untouched(run, name, case, plan_kw, dp):
    check_fallback(run, case, plan_kw, dp)


@pytest.mark.parametrize("which", ["frequency", "input-buffer"])
def test_special_fallbacks_untouched(run, which):
    check_special_fallback(run, which)


# ---- device -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_plan_shape(grun):
    check_plan_shape(grun)


@pytest.mark.gpu
@pytest.mark.parametrize("dp,group", GROUPS, ids=GROUP_IDS)
def test_gpu_every_instance(grun, dp, group):
    for n in group:
        check_instance(grun, n, dp)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,r2c", WIDTHS, ids=WIDTH_IDS)
def test_gpu_narrow_and_exact_widths(grun, shape, r2c):
    check_width(grun, shape, r2c)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,nb,r2c", VOLUMES, ids=VOLUME_IDS)
def test_gpu_three_dimensions(grun, shape, nb, r2c):
    check_volume(grun, shape, nb, r2c)


@pytest.mark.gpu
@pytest.mark.parametrize("cf", [2, 3])
@pytest.mark.parametrize("dp", [False, True], ids=["fp32", "fp64"])
def test_gpu_coordinates(grun, dp, cf):
    check_coordinates(grun, cf, dp)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,r2c,dp", CONJ, ids=CONJ_IDS)
def test_gpu_conjugation(grun, mode, r2c, dp):
    check_conjugation(grun, mode, r2c, dp)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,pads,r2c,dp", PADS, ids=PAD_IDS)
def test_gpu_zero_padding(grun, shape, pads, r2c, dp):
    check_zero_padding(grun, shape, pads, r2c, dp)


@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
def test_gpu_launch_parameters(grun, r2c):
    check_launch_parameters(grun, r2c)


@pytest.mark.gpu
def test_gpu_plain_inverse_of_a_merged_application(grun):
    check_plain_inverse(grun)


@pytest.mark.gpu
@pytest.mark.parametrize("name,case,plan_kw,dp", FALLBACKS, ids=FALLBACK_IDS)
def test_gpu_fallbacks_untouched(grun, name, case, plan_kw, dp):
    check_fallback(grun, case, plan_kw, dp)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["frequency", "input-buffer"])
def test_gpu_special_fallbacks_untouched(grun, which):
    check_special_fallback(grun, which)

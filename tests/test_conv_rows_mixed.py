"""One-launch 1-D convolution on 7-smooth rows that are no power of two (mix_conv_row_kernel, kernel_mix_conv.h): forward transform, kernel product and inverse
transform of unit-stride rows of 100 ... 4096 points (fp64: ... 2048) in one kernel.  The same checks run on the CPU emulator build (unmarked) and on the device
(pytest.mark.gpu).  Truth is numpy in double precision (test_conv_rows.row_case); bounds are those of the existing convolution tests: relative L2 < 6e-5 in fp32,
< 1e-12 in fp64.  The length lists are derived here from the rule, not read from the generated table: a missing table entry fails."""
import ctypes as C
import re

import numpy as np
import pytest

import convpad
from helpers import Runner, rel_l2
from test_conv_rows import bound, row_case, separate_passes
from vkfft_amd import api

KERNEL = "mix_conv_row_kernel"
FUSED = (1, KERNEL)
SLOTS = 197  # prime: every FPW from 2 to 64 gets at least three full tiles and a partial one


def smooth7(n):
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def lengths(dp, r2c):
    """the rule of the instance table: 7-smooth, no power of two, 100 ... 4096 (fp64: 2048), even for pairs of real rows"""
    return [n for n in range(100, (2048 if dp else 4096) + 1) if smooth7(n) and n & (n - 1) and not (r2c and n % 2)]


def _chunks(seq, size):
    return [seq[i:i + size] for i in range(0, len(seq), size)]


# groups of at most 40 instances: (dp, r2c, lengths)
GROUPS = [(dp, r2c, chunk) for dp in (False, True) for r2c in (False, True) for chunk in _chunks(lengths(dp, r2c), 40)]
GROUP_IDS = [f"{'fp64' if dp else 'fp32'}-{'r2c' if r2c else 'c2c'}-{chunk[0]}-{chunk[-1]}" for dp, r2c, chunk in GROUPS]

# every radix, every stage count, both load forms, odd lengths
SAMPLE32 = [100, 105, 120, 144, 192, 243, 250, 343, 360, 625, 729, 1000, 1080, 1296, 1536, 2000, 2187, 2401, 3000, 3125, 3600, 3969, 4000, 4032]
SAMPLE64 = [100, 360, 1000, 2000]
SAMPLE = ([(n, False, False) for n in SAMPLE32] + [(n, False, True) for n in SAMPLE32 if n % 2 == 0] +
          [(n, True, False) for n in SAMPLE64 + [243, 625]] + [(n, True, True) for n in SAMPLE64])
SAMPLE_IDS = [f"{n}-{'fp64' if dp else 'fp32'}-{'r2c' if r2c else 'c2c'}" for n, dp, r2c in SAMPLE]


def test_the_rule_gives_the_documented_instance_counts():
    assert [len(lengths(dp, r2c)) for dp in (False, True) for r2c in (False, True)] == [197, 154, 140, 108]
    assert all(len(g[2]) <= 40 for g in GROUPS)


def _plan_names(run, shape, nb=1, **kw):
    """(launches, names) of a convolution plan that is only planned (buffers of one page: never run)"""
    hk, pk = run._alloc(np.zeros(512, np.float64)); hd, pd = run._alloc(np.zeros(512, np.float64))
    app = api.App(list(shape), nb, buffer_ptr=pd, kernel=pk, performConvolution=1, lib=run.lib, normalize=True, **kw)
    buf = C.create_string_buffer(1024)
    n = run.lib.vkfftMI355XDescribePlan(C.byref(app.app), 0, buf, 1024)
    app.delete()
    return int(n), [x.split("<")[0] for x in buf.value.decode().split(",") if x]


def reported_fpw(run, capfd, n, dp, r2c):
    """rows (pairs of real rows) per workgroup as the plan's print-plan line reports them"""
    capfd.readouterr()
    info = _plan_names(run, (n,), dp=dp, r2c=r2c, printMemoryLayout=1)
    m = re.search(KERNEL + r", (\d+) rows per workgroup", capfd.readouterr().err)
    assert m, info
    return int(m.group(1))


# ---- the checks: the emulator and the device run the same functions ------------------------------------------------

def check_plan_shape(run):
    for n, r2c, dp in ((1000, False, False), (360, True, True)):
        a = row_case(run, n, nb=3, r2c=r2c, dp=dp)
        assert a["info"] == FUSED, a["info"]
        assert a["err"] < bound(dp), a["err"]
        b = row_case(run, n, nb=3, r2c=r2c, dp=dp, separate=True)
        assert b["info"][0] == 3, b["info"]
        assert b["err"] < bound(dp), b["err"]
        with separate_passes():
            launches, names = _plan_names(run, (n,), nb=3, dp=dp, r2c=r2c)
        assert launches == 3 and "conv_pointwise_kernel" in names and KERNEL not in names, (launches, names)


def check_instance(run, n, dp, r2c, slots=SLOTS):
    """coordinateFeatures = 1; C2C: `slots` batches; R2C: 2 slots - 1 batches, so the last one is unpaired"""
    a = row_case(run, n, cf=1, nb=2 * slots - 1 if r2c else slots, r2c=r2c, dp=dp, seed=n)
    tag = (n, dp, r2c)
    assert a["info"] == FUSED, (tag, a["info"])
    print(f"N={n} {'fp64' if dp else 'fp32'} {'r2c' if r2c else 'c2c'}: rel L2 {a['err']:.3e}")
    assert a["err"] < bound(dp), (tag, a["err"])
    assert a["kernel_untouched"], (tag, "the kernel buffer was written")
    assert a["tail_untouched"], (tag, "a row behind the last one was written")
    assert a.get("pad_reals_untouched", True), (tag, "the padding reals of a row were written")


def check_coordinates(run, n, dp, r2c, cf):
    """11 batches: 22 / 33 rows, more than three tiles of the largest FPW among these shapes (7) and a partial one; R2C: an unpaired last batch"""
    a = row_case(run, n, cf=cf, nb=11, r2c=r2c, dp=dp, seed=11 + cf)
    assert a["info"] == FUSED, a["info"]
    assert a["err"] < bound(dp), a["err"]
    assert a["kernel_untouched"] and a["tail_untouched"] and a.get("pad_reals_untouched", True)


def check_conjugation(run, dp, mode):
    a = row_case(run, 120, cf=2, nb=30, dp=dp, conjugate=mode, seed=mode)
    assert a["info"] == FUSED, a["info"]
    assert a["err"] < bound(dp), a["err"]


def check_r2c_conjugate_keeps_three_launches(run):
    for mode in (1, 2):
        a = row_case(run, 120, cf=2, nb=3, r2c=True, conjugate=mode)
        assert a["info"][0] == 3 and a["info"][1] != KERNEL, a["info"]
        assert a["err"] < bound(False), a["err"]


def check_zero_padding(run, n, pad, r2c, dp):
    a = row_case(run, n, cf=2, nb=5, r2c=r2c, dp=dp, pad=pad, seed=7)
    assert a["info"] == FUSED, a["info"]
    assert a["err"] < bound(dp), a["err"]
    # the padded range of the result is not stored: it keeps the NaN it held on entry
    assert np.isnan(a["got"][:10, pad[0]:pad[1]]).all()
    assert a["kernel_untouched"] and a["tail_untouched"] and a.get("pad_reals_untouched", True)


def check_launch_parameters(run, r2c):
    a = row_case(run, 600, cf=2, nb=5, r2c=r2c, at_launch=True, seed=9)
    assert a["info"] == FUSED, a["info"]
    assert a["err"] < bound(False), a["err"]
    assert a["kernel_untouched"] and a["tail_untouched"]


def check_plain_inverse(run):
    rng = np.random.default_rng(5)
    x = (rng.uniform(-1, 1, (3, 120)) + 1j * rng.uniform(-1, 1, (3, 120))).astype(np.complex64)
    hk, pk = run._alloc(np.ones(120, np.complex64))
    hd, pd = run._alloc(x)
    ca = api.App([120], 3, buffer_ptr=pd, performConvolution=1, kernel=pk, lib=run.lib, normalize=True)
    assert ca.launch_info() == FUSED
    ca.inverse()
    got = run._fetch(hd, np.complex64).reshape(x.shape)
    n_launch, name = ca.launch_info(inverse=True)
    ca.delete()
    assert n_launch >= 1 and name != KERNEL
    assert rel_l2(got, np.fft.ifft(x.astype(np.complex128), axis=-1)) < 2e-6


def check_agrees_with_separate_passes(run, n, dp, r2c):
    """both paths hold the bound against the truth, so they lie within twice the bound of each other"""
    kw = dict(cf=2, nb=9, r2c=r2c, dp=dp, seed=n)
    a = row_case(run, n, **kw)
    b = row_case(run, n, separate=True, **kw)
    assert a["info"] == FUSED and b["info"][0] == 3, (a["info"], b["info"])
    print(f"N={n}: one launch {a['err']:.3e}, three launches {b['err']:.3e}")
    assert a["err"] < bound(dp) and b["err"] < bound(dp), (a["err"], b["err"])
    assert rel_l2(a["got"][:18, :n], b["got"][:18, :n]) < 2 * bound(dp)


# (what conv_case runs, what the plan is created with, double precision)
FALLBACKS = [
    ("n96", dict(shape=(96,), nb=2), dict(nb=2), False),
    ("n4095-factor-13", dict(shape=(4095,), nb=2), dict(nb=2), False),
    ("n4200-above-the-range", dict(shape=(4200,), nb=2), dict(nb=2), False),
    ("fp64-n2160", dict(shape=(2160,), nb=2, dp=True), dict(nb=2, dp=True), True),
    # (one row: convpad.conv_case lays real rows out N + 2 reals apart, the pitch of an even length; an odd length has N + 1)
    ("r2c-n225-odd", dict(shape=(225,), r2c=True), dict(r2c=True), False),
    ("matrix2", dict(shape=(1000,), m=2), dict(matrixConvolution=2, coordinateFeatures=2), False),
    ("two-kernels", dict(shape=(1000,), nk=2), dict(numberKernels=2), False),
    ("cross-power", dict(shape=(1000,), cf=2, cross=True), dict(coordinateFeatures=2, crossPowerSpectrumNormalization=1), False),
    ("2d-1000x8", dict(shape=(1000, 8), nb=2), dict(nb=2), False),
]
FALLBACK_IDS = [f[0] for f in FALLBACKS]


def check_fallback(run, case, plan_kw, dp):
    c = dict(case); shape = c.pop("shape")
    err = convpad.conv_case(run, shape, **c)
    assert err < bound(dp), err
    launches, names = _plan_names(run, shape, **dict(plan_kw))
    assert launches >= 3 and KERNEL not in names, (launches, names)


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


COORDS = [(1000, False, False), (360, True, False), (1200, False, True)]
COORD_IDS = ["1000-fp32-c2c", "360-fp64-c2c", "1200-fp32-r2c"]
PADS = [(1000, (500, 1000), False), (360, (90, 200), True), (4000, (2000, 4000), False)]  # (the middle one in fp64)
PAD_IDS = [f"{n}-{p[0]}-{p[1]}" for n, p, _ in PADS]
AGREE = [(360, False, False), (4000, False, True), (1000, True, False)]
AGREE_IDS = ["360-fp32-c2c", "4000-fp32-r2c", "1000-fp64-c2c"]


def test_plan_shape(run):
    check_plan_shape(run)


@pytest.mark.parametrize("n,dp,r2c", SAMPLE, ids=SAMPLE_IDS)
def test_every_instance_class(run, n, dp, r2c):
    """(197 slots here too: the emulator needs well under a second for the longest of them)"""
    check_instance(run, n, dp, r2c)


@pytest.mark.parametrize("cf", [2, 3])
@pytest.mark.parametrize("n,dp,r2c", COORDS, ids=COORD_IDS)
def test_coordinates(run, n, dp, r2c, cf):
    check_coordinates(run, n, dp, r2c, cf)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("dp", [False, True], ids=["fp32", "fp64"])
def test_conjugation(run, dp, mode):
    check_conjugation(run, dp, mode)


def test_r2c_with_conjugation_keeps_three_launches(run):
    check_r2c_conjugate_keeps_three_launches(run)


@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
@pytest.mark.parametrize("n,pad,dp", PADS, ids=PAD_IDS)
def test_zero_padding(run, n, pad, dp, r2c):
    check_zero_padding(run, n, pad, r2c, dp)


@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
def test_launch_parameters(run, r2c):
    check_launch_parameters(run, r2c)


def test_plain_inverse_of_a_fused_application(run):
    check_plain_inverse(run)


@pytest.mark.parametrize("n,dp,r2c", AGREE, ids=AGREE_IDS)
def test_fused_agrees_with_separate_passes(run, n, dp, r2c):
    check_agrees_with_separate_passes(run, n, dp, r2c)


@pytest.mark.parametrize("name,case,plan_kw,dp", FALLBACKS, ids=FALLBACK_IDS)
def test_fallbacks_untouched(run, name, case, plan_kw, dp):
    check_fallback(run, case, plan_kw, dp)


# ---- device -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_plan_shape(grun):
    check_plan_shape(grun)


@pytest.mark.gpu
@pytest.mark.parametrize("dp,r2c,group", GROUPS, ids=GROUP_IDS)
def test_gpu_every_instance(grun, dp, r2c, group):
    for n in group:
        check_instance(grun, n, dp, r2c)


@pytest.mark.gpu
@pytest.mark.parametrize("cf", [2, 3])
@pytest.mark.parametrize("n,dp,r2c", COORDS, ids=COORD_IDS)
def test_gpu_coordinates(grun, n, dp, r2c, cf):
    check_coordinates(grun, n, dp, r2c, cf)


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
@pytest.mark.parametrize("n,pad,dp", PADS, ids=PAD_IDS)
def test_gpu_zero_padding(grun, n, pad, dp, r2c):
    check_zero_padding(grun, n, pad, r2c, dp)


@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [False, True], ids=["c2c", "r2c"])
def test_gpu_launch_parameters(grun, r2c):
    check_launch_parameters(grun, r2c)


@pytest.mark.gpu
def test_gpu_plain_inverse_of_a_fused_application(grun):
    check_plain_inverse(grun)


@pytest.mark.gpu
@pytest.mark.parametrize("n,dp,r2c", AGREE, ids=AGREE_IDS)
def test_gpu_fused_agrees_with_separate_passes(grun, n, dp, r2c):
    check_agrees_with_separate_passes(grun, n, dp, r2c)


@pytest.mark.gpu
def test_gpu_many_tiles(grun, capfd):
    """more tiles than a device holds at once: FPW * (8 per compute unit + 1) rows of 100 points; the per-row error shows a tile that was skipped or done twice"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = reported_fpw(grun, capfd, 100, False, False) * (8 * cus + 1)
    rng = np.random.default_rng(1)
    kern = (rng.uniform(-1, 1, 100) + 1j * rng.uniform(-1, 1, 100)).astype(np.complex64)
    data = (rng.uniform(-1, 1, (rows, 100)) + 1j * rng.uniform(-1, 1, (rows, 100))).astype(np.complex64)
    want = np.fft.ifft(np.fft.fft(kern.astype(np.complex128))[None] * np.fft.fft(data.astype(np.complex128), axis=-1), axis=-1)
    hk, pk = grun._alloc(kern); hd, pd = grun._alloc(data)
    common = dict(lib=grun.lib, normalize=True)
    ka = api.App([100], 1, buffer_ptr=pk, kernelConvolution=1, **common); ka.forward(); ka.delete()
    ca = api.App([100], rows, buffer_ptr=pd, kernel=pk, performConvolution=1, **common)
    assert ca.launch_info() == FUSED
    ca.forward()
    got = grun._fetch(hd, np.complex64).reshape(data.shape)
    ca.delete()
    assert rel_l2(got, want) < bound(False)
    per_row = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    assert per_row.max() < 10 * bound(False), (int(per_row.argmax()), float(per_row.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name,case,plan_kw,dp", FALLBACKS, ids=FALLBACK_IDS)
def test_gpu_fallbacks_untouched(grun, name, case, plan_kw, dp):
    check_fallback(grun, case, plan_kw, dp)

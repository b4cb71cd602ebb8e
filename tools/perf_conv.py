"""Convolution throughput next to the reference on the same box (same call): python tools/perf_conv.py  ->  JSON lines.
Algorithmic bytes of one convolution append = read + write of the data systems + one read of the kernel systems.
python tools/perf_conv.py rows: one-dimensional plans, the one-launch form (pow2_conv_row_kernel, mix_conv_row_kernel) against VKFFT_MI355X_CONV_SEPARATE=1 (three
launches) in the same process, alternating, on one buffer of 256 MiB; beside them the plain transform of the same rows (forward and normalised inverse in turn): the
ceiling of a kernel that reads and writes the data once.
python tools/perf_conv.py planes: 2-D / 3-D plans whose last axis is 7-smooth and no power of two, the merged last axis (mix_conv_col_kernel: three launches for a
2-D plan) against VKFFT_MI355X_CONV_SEPARATE=1 (five) in the same process, alternating, on the same buffer; and the bank cases, one input against numberKernels = K
kernels (mix_conv_col_bank_kernel, pow2_col_blue_kernel MODE 9): one batch, a buffer of K systems."""
import ctypes as C, json, os, sys, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np, torch
from vkfft_amd import api


def rows_ab(n, dp, r2c, pad, mib=256, rounds=7, it=10):
    """fused against separate passes: `rounds` alternating windows of `it` appends each, timed with device events; the kernel spectrum is all ones (the data stays
    what it is however often the convolution runs)"""
    rb = (n + 2 if r2c else 2 * n) * (8 if dp else 4)
    rows = (mib << 20) // rb
    rt = torch.float64 if dp else torch.float32
    data = torch.rand((mib << 20) // (8 if dp else 4), device="cuda", dtype=rt)
    kern = torch.zeros(2 * n + 4, device="cuda", dtype=rt); kern[0::2] = 1
    kw = dict(buffer_ptr=data.data_ptr(), kernel=kern.data_ptr(), performConvolution=1, dp=dp, r2c=r2c, normalize=True)
    if pad:
        kw.update(performZeropadding=[1, 0, 0, 0], fft_zeropad_left=[n // 2, 0, 0, 0], fft_zeropad_right=[n, 0, 0, 0])
    apps = {}
    apps["fused"] = api.App([n], rows, **kw)
    os.environ["VKFFT_MI355X_CONV_SEPARATE"] = "1"
    try:
        apps["separate"] = api.App([n], rows, **kw)
    finally:
        del os.environ["VKFFT_MI355X_CONV_SEPARATE"]
    info = {k: a.launch_info() for k, a in apps.items()}
    apps["plain"] = api.App([n], rows, buffer_ptr=data.data_ptr(), dp=dp, r2c=r2c, normalize=True)  # (no padding: the whole rows)
    plain_kernel = apps["plain"].launch_info()[1]
    def run(k, a, i):
        if k == "plain" and i % 2: a.inverse()
        else: a.forward()
    for k, a in apps.items():
        for i in range(4): run(k, a, i)
    torch.cuda.synchronize()
    ms = {k: [] for k in apps}
    for _ in range(rounds):
        for k, a in apps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(it): run(k, a, i)
            e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / it)
    for a in apps.values(): a.delete()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    moved = 2 * rows * rb * (0.5 if pad else 1.0)  # bytes the algorithm owes: one read and one write of the (unpadded part of the) data
    return dict(n=n, dp=dp, r2c=r2c, zero_padded_upper_half=bool(pad), rows=rows, launches={k: v[0] for k, v in info.items()}, kernel=info["fused"][1],
                ms={k: round(v, 4) for k, v in med.items()}, ms_min_max={k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                fused_alg_GBps=round(moved / med["fused"] / 1e6, 1), separate_alg_GBps=round(moved / med["separate"] / 1e6, 1),
                plain_kernel=plain_kernel, plain_GBps=round(2 * rows * rb / med["plain"] / 1e6, 1),
                speedup=round(med["separate"] / med["fused"], 3), separate_spread=round((max(ms["separate"]) - min(ms["separate"])) / med["separate"], 3))


def planes_ab(shape, dp, r2c, pad, nk=1, mib=256, rounds=7, it=10):
    """merged last axis against separate passes, timed like rows_ab.  shape: axis 0 first, the merged axis last; as many batches as fit `mib` (at least one).
    nk > 1: a bank of nk kernels, ONE batch (the library takes no bank together with several batches) in a buffer of nk systems, whatever its size"""
    es = 16 if dp else 8
    elems = (shape[0] // 2 + 1 if r2c else shape[0]) * int(np.prod(shape[1:]))
    nb = max(1, (mib << 20) // (elems * es)) if nk == 1 else 1
    rt = torch.float64 if dp else torch.float32
    data = torch.rand(2 * elems * nb * nk, device="cuda", dtype=rt)
    kern = torch.zeros(2 * elems * nk, device="cuda", dtype=rt); kern[0::2] = 1
    kw = dict(buffer_ptr=data.data_ptr(), kernel=kern.data_ptr(), performConvolution=1, dp=dp, r2c=r2c, normalize=True)
    if nk > 1:
        kw.update(numberKernels=nk)
    last = len(shape) - 1
    if pad:
        flag = [0] * 4; left = [0] * 4; right = [0] * 4
        flag[last], left[last], right[last] = 1, shape[last] // 2, shape[last]
        kw.update(performZeropadding=flag, fft_zeropad_left=left, fft_zeropad_right=right)
    apps = {}
    apps["merged"] = api.App(list(shape), nb, **kw)
    os.environ["VKFFT_MI355X_CONV_SEPARATE"] = "1"
    try:
        apps["separate"] = api.App(list(shape), nb, **kw)
    finally:
        del os.environ["VKFFT_MI355X_CONV_SEPARATE"]
    info = {k: a.launch_info() for k, a in apps.items()}
    buf = C.create_string_buffer(2048)
    apps["merged"].lib.vkfftMI355XDescribePlan(C.byref(apps["merged"].app), 0, buf, 2048)
    names = sorted(set(x.split("<")[0] for x in buf.value.decode().split(",") if x))
    for a in apps.values():
        for i in range(4): a.forward()
    torch.cuda.synchronize()
    ms = {k: [] for k in apps}
    for _ in range(rounds):
        for k, a in apps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(it): a.forward()
            e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / it)
    for a in apps.values(): a.delete()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    moved = (1 + nk) * nb * elems * es  # one read of the data and one write per result (the padded half included: the other axes visit it)
    return dict(shape=list(shape), dp=dp, r2c=r2c, zero_padded_upper_half_of_last_axis=bool(pad), batches=nb, kernels=nk, buffer_MiB=round(nb * nk * elems * es / 2**20, 1), launches={k: v[0] for k, v in info.items()}, merged_kernels=names,
                ms={k: round(v, 4) for k, v in med.items()}, ms_min_max={k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                merged_alg_GBps=round(moved / med["merged"] / 1e6, 1), separate_alg_GBps=round(moved / med["separate"] / 1e6, 1),
                speedup=round(med["separate"] / med["merged"], 3), separate_spread=round((max(ms["separate"]) - min(ms["separate"])) / med["separate"], 3))


if len(sys.argv) > 1 and sys.argv[1] == "planes":
    print(json.dumps(dict(source_hash=api.source_hash(), library_is_current=api.library_is_current(), device=torch.cuda.get_device_name(0))), flush=True)
    for shape, dp, r2c, pad in [((1920, 1080), False, False, False), ((1000, 1000), False, False, False), ((360, 360, 360), False, False, False), ((360, 360, 360), False, True, False),
                                ((1024, 1536), False, False, False), ((480, 500), True, False, False), ((1920, 1080), False, False, True)]:
        print(json.dumps(planes_ab(shape, dp, r2c, pad)), flush=True)
    # banks of kernels.  Last axes of 1080 and 1000 points have no bank instance (tools/gen_mix_conv_col_bank_table.py, DROPPED): both sides run the separate passes
    for shape, dp, r2c, pad, nk in [((1920, 1080), False, False, False, 2), ((1920, 1080), False, False, False, 8), ((1000, 1000), False, False, False, 4), ((360, 360, 360), False, True, False, 2),
                                    ((480, 500), True, False, False, 4), ((1024, 1024), False, False, False, 4), ((1920, 1080), False, False, True, 4),
                                    # the classes the cases above leave out (fp32 tiles of 8 / 16 / 32 columns on lengths that have an instance, a second fp64 length, the power-of-two form in fp64)
                                    ((1920, 1200), False, False, False, 2), ((1920, 1200), False, False, False, 8), ((1920, 1200), False, False, True, 4), ((1000, 720), False, False, False, 4),
                                    ((1000, 120), False, False, False, 4), ((480, 120), True, False, False, 4), ((1024, 1024), True, False, False, 4)]:
        print(json.dumps(planes_ab(shape, dp, r2c, pad, nk)), flush=True)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "rows":
    print(json.dumps(dict(source_hash=api.source_hash(), library_is_current=api.library_is_current(), device=torch.cuda.get_device_name(0))), flush=True)
    for n, dp, r2c, pad in [(256, False, False, False), (1024, False, False, False), (4096, False, False, False), (256, False, True, False), (1024, False, True, False),
                            (4096, False, True, False), (1024, True, False, False), (1024, True, True, False), (1024, False, False, True), (4096, False, True, True),
                            # 7-smooth rows (mix_conv_row_kernel): the short ones move their tile as one contiguous run, the others load and store in the transforms
                            (100, False, False, False), (200, False, False, False), (360, False, False, False), (1000, False, False, False), (3000, False, False, False),
                            (4000, False, False, False), (100, False, True, False), (360, False, True, False), (1000, False, True, False), (3000, False, True, False),
                            (4000, False, True, False), (100, True, False, False), (1000, True, False, False), (100, True, True, False), (1000, True, True, False),
                            (4000, False, False, True), (4000, False, True, True)]:
        print(json.dumps(rows_ab(n, dp, r2c, pad)), flush=True)
    sys.exit(0)
ref = None
p = os.path.join(root, "oracle", "_ref", "libvkfft_ref.so")
if os.path.exists(p):
    ref = C.CDLL(p); ref.ref_convolution.restype = C.c_int
for shape, m, r2c in [((4096, 4096), 1, False), ((2048, 2048), 3, False), ((4096, 4096), 1, True), ((1024, 1024), 3, True)]:
    cf = m; ksys = m * m
    elems = (shape[0] // 2 + 1 if r2c else shape[0]) * shape[1]
    kbytes, dbytes = ksys * elems * 8, cf * elems * 8
    kern = torch.randn(kbytes // 4, device="cuda"); data = torch.randn(dbytes // 4, device="cuda")
    ka = api.App(list(shape), 1, buffer_ptr=kern.data_ptr(), coordinateFeatures=ksys, kernelConvolution=1, r2c=r2c, normalize=True)
    ka.forward()
    ca = api.App(list(shape), 1, buffer_ptr=data.data_ptr(), coordinateFeatures=cf, performConvolution=1, matrixConvolution=m, kernel=kern.data_ptr(), r2c=r2c, normalize=True)
    for _ in range(3): ca.forward()
    torch.cuda.synchronize(); t0 = time.perf_counter(); it = 20
    for _ in range(it): ca.forward()
    torch.cuda.synchronize(); ms = (time.perf_counter() - t0) / it * 1e3
    ka.delete(); ca.delete()
    out = dict(shape=shape, matrix=m, r2c=r2c, ms=round(ms, 4), alg_GBps=round((2 * dbytes + kbytes) / ms / 1e6, 1))
    if ref is not None:
        hk = np.random.default_rng(0).uniform(-1, 1, kbytes // 4).astype(np.float32); hd = np.random.default_rng(1).uniform(-1, 1, dbytes // 4).astype(np.float32)
        rms = C.c_double(0)
        rc = ref.ref_convolution(2, (C.c_uint64 * 4)(*shape), int(r2c), 0, C.c_uint64(cf), C.c_uint64(m), C.c_uint64(1), 0, 0, 0, C.c_uint64(ksys), hk.ctypes.data_as(C.c_void_p),
                                 C.c_uint64(kbytes), hd.ctypes.data_as(C.c_void_p), C.c_uint64(dbytes), C.byref(rms), 20)
        out.update(ref_rc=rc, ref_ms=round(rms.value, 4), ratio_vs_ref=round(rms.value / ms, 2) if rc == 0 else None)
    print(json.dumps(out), flush=True)

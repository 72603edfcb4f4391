"""The fp32 implicit-filter kernels (csrc/filter_kernels.h: filter_fwd_kernel, filter_layer_bwd_kernel in its six instantiations,
filter_reduce_kernel, filter_reduce_multi_kernel, filter_compact_kernel) on the CPU-emulated build, element by element against the layer-local
fp64 references of tests/filter_local.py: every saved pre-activation and filter tap, every element of delta_1, delta_0, dz and of every
parameter gradient against a bound derived from fp32 arithmetic, pad columns and poisoned buffers, bit-identity of the SAVE templates, of
repeated calls and of the call without dz.  The cases are the smallest shapes that reach each branch (profiles/filter_local.md has the table
and the measured figures); the same checks run on the gfx950 library in tests/test_gpu_filter_local.py."""
import ctypes

import pytest
import torch

from oracle import hyena_oracle as O
from tests import filter_local as FLoc
from tests.test_filter_emu import NAMES, _make_filter

# (D, L, E, ldk or None, z_stride or None, shift, grid, the `count` of each reduction)
CASES = [
    (64, 1, 1, None, None, 0.0, 1, {"dw3": 2, "dw2": 2, "dw1": 2, "dw0": 4, "db2": 4, "db1": 4, "db0": 8, "dfreq": 8}),
    (128, 31, 3, None, None, 0.05, 1, {"dw3": 1, "dw2": 2, "dw1": 2, "dw0": 4, "db2": 4, "db1": 4, "db0": 8, "dfreq": 8}),
    (64, 257, 8, None, None, 0.0, 2, {"dw3": 4, "dw2": 4, "dw1": 4, "dw0": 8, "db2": 8, "db1": 8, "db0": 16, "dfreq": 16}),
    (256, 300, 5, None, None, 0.05, 2, {"dw3": 2, "dw2": 4, "dw1": 4, "dw0": 8, "db2": 8, "db1": 8, "db0": 16, "dfreq": 16}),
    (256, 300, 5, 301, None, 0.05, 2, None),
    (256, 300, 5, 304, None, 0.05, 2, None),
    (128, 1000, 2, None, None, 0.0, 4, {"dw3": 4, "dw2": 8, "dw1": 8, "dw0": 16, "db2": 16, "db1": 16, "db0": 32, "dfreq": 32}),
    (64, 1023, 7, None, None, 0.05, 4, {"dw3": 8, "dw2": 8, "dw1": 8, "dw0": 16, "db2": 16, "db1": 16, "db0": 32, "dfreq": 32}),
    (64, 130, 5, None, 8, 0.05, 1, None),
]
# the reduction kernels at their own edges (GPU file: all three; here: those the emulator runs in well under 20 s)
LONG_CASES = [
    (256, 4096, 5, None, None, 0.05, 16, {"dw3": 16, "dw2": 32, "dw1": 32, "dw0": 64, "db2": 64, "db1": 64, "db0": 128, "dfreq": 128}),
    (256, 4099, 5, None, None, 0.0, 17, {"dw3": 17, "dw2": 34, "dw1": 34, "dw0": 68, "db2": 68, "db1": 68, "db0": 136, "dfreq": 136}),
]
HUGE_CASE = (64, 65799, 4, None, None, 0.05, 256, {"dw3": 512, "dw2": 512, "dw1": 512, "dw0": 1024, "db2": 1024, "db1": 1024, "db0": 2048, "dfreq": 2048})


def check_counts(D, L, grid, counts):
    """the `count` each reduction of this case sees, from L, KS and the grid: a change of the grid policy must not move a case off its edge"""
    assert FLoc.grid_of(L) == grid
    assert (FLoc.KS(64, 64), FLoc.KS(128, 64), FLoc.KS(256, 64), FLoc.KS(64, 8)) == (2, 1, 1, 4)
    if counts is not None:
        assert FLoc.reduction_counts(D, L) == counts
    if (D, L) == (256, 4096):       # count = 128: every thread row takes the unrolled loop exactly once, no tail
        assert FLoc.reduce_loops(128) == (16, 1, 0)
    if (D, L) == (256, 4099):       # 136: all rows unrolled once, rows 0 .. 7 a tail; 68 / 34 / 17: rows skip the unrolled loop, tail only
        assert FLoc.reduce_loops(136) == (16, 1, 8) and FLoc.reduce_loops(68) == (0, 0, 16) and FLoc.reduce_loops(17) == (0, 0, 16)
    if (D, L) == (64, 65799):       # 258 workgroup iterations on 256 workgroups, ragged last tile
        assert (L + 255) // 256 == 258 and L % 32 == 7
        assert FLoc.reduce_loops(2048) == (16, 16, 0) and FLoc.reduce_loops(512) == (16, 4, 0)


def run_case(_lib, case, device="cpu", label="emu", **kw):
    D, L, E, ldk, zs, shift, grid, counts = case
    check_counts(D, L, grid, counts)
    args = FLoc.make_case(D, L, E, seed=D + L + E, shift=shift, z_stride=zs, device=device)
    dk = torch.randn(D, L, generator=torch.Generator().manual_seed(1)).to(device)
    return FLoc.check_local(_lib, args, shift, kw.pop("modulate", True), dk, ldk=ldk, label=label, **kw)


@pytest.mark.parametrize("case", CASES + LONG_CASES, ids=lambda c: f"D{c[0]}-L{c[1]}-E{c[2]}-ldk{c[3]}-zs{c[4]}")
def test_filter_layer_local_vs_fp64(emu_backend, case):
    run_case(emu_backend, case)


@pytest.mark.parametrize("kw", [{"modulate": False}, {"need_dz": False}], ids=["nomod", "nodz"])
def test_filter_layer_local_strided_z_options(emu_backend, kw):
    """z_stride = 8 > E = 5 with NaN in the unused columns, without the modulation and without dz"""
    run_case(emu_backend, CASES[-1], **kw)


def test_modulation_probe(emu_backend):
    """eps_m through the ABI: what a 1 - 2 ulp exp2 explains (2 ulp of a value at the bottom of its binade = 4 u)"""
    eps, info = FLoc.modulation_probe(emu_backend, torch.device("cpu"))
    print(f"[filter-local] emu eps_m measured {eps:.3g} = {eps / FLoc.U:.2f} u; {info}")
    assert info["samples"] > 0.5 * 256 * 2048 and info["max_t_delta"] > 80
    assert eps <= FLoc.EPS_M_CAP, eps


def test_hy_sincos_error_is_the_sigma_of_the_bounds(emu_backend):
    """sigma of tests/filter_local.py is twice the largest absolute error of hy_sincos over |x| <= SINCOS_RANGE, measured here"""
    lib = emu_backend.lib()
    lib.hipemu_probe_sincos.restype = None
    lib.hipemu_probe_sincos.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    X = FLoc.SINCOS_RANGE
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.linspace(-X, X, (1 << 22) + 1, dtype=torch.float64).float(),
                   (torch.rand(1 << 20, generator=g, dtype=torch.float64) * 2 - 1).mul(32).float(), torch.tensor([0.0, -0.0, X, -X])]).contiguous()
    sn, cs = torch.empty_like(x), torch.empty_like(x)
    lib.hipemu_probe_sincos(x.data_ptr(), sn.data_ptr(), cs.data_ptr(), x.numel())
    err = max((sn.double() - torch.sin(x.double())).abs().max().item(), (cs.double() - torch.cos(x.double())).abs().max().item())
    print(f"[filter-local] hy_sincos max abs error {err:.4g}; sigma = {FLoc.SIGMA:.4g}")
    assert err <= FLoc.SIGMA_MEASURED * 1.001 and FLoc.SIGMA == 2 * FLoc.SIGMA_MEASURED


@pytest.mark.parametrize("D,L,emb_dim,shift", [(64, 300, 5, 0.0), (128, 77, 3, 0.05), (256, 130, 7, 0.0)])
def test_fp64_backward_reference_is_the_oracles_autograd(monkeypatch, D, L, emb_dim, shift):
    """backward_ref, fed the ORACLE'S fp64 pre-activations, reproduces autograd's gradients of oracle.hyena_oracle.hyena_filter to 1e-12: the
    reference the kernels are held to does not depend on any kernel"""
    f = _make_filter(D, L, emb_dim=emb_dim, seed=D + L, shift=shift)
    dk = torch.randn(D, L, generator=torch.Generator().manual_seed(1))
    acts = []

    class RecordingF:
        @staticmethod
        def linear(h, w, b=None):
            out = torch.nn.functional.linear(h, w, b)
            acts.append(out.detach())
            return out
    monkeypatch.setattr(O, "F", RecordingF)
    sd = {"filter_fn." + k: v.detach().double().requires_grad_(v.dtype.is_floating_point) for k, v in f.state_dict().items()}
    k = O.hyena_filter(sd, L, shift=shift)[0].transpose(0, 1)
    k.backward(dk.double())
    monkeypatch.undo()
    assert len(acts) == 4 and all(a.dtype == torch.float64 and a.shape == (1, L, 64) for a in acts[:3])
    args, sh, modulate = FLoc.module_args(f, L)
    assert sh == shift and modulate
    args64 = [a.double() for a in args]                             # fp64 everywhere: x = freq a is then exact in both
    g, _ = FLoc.backward_ref(dk, [a[0].t().contiguous() for a in acts[:3]], args64, shift, modulate)
    for name, key in zip(NAMES, ("dz", "dw0", "db0", "dw1", "db1", "dw2", "db2", "dw3", "dfreq")):
        ref = sd["filter_fn." + name].grad
        if name.endswith("freq"):
            ref = sum(sd[f"filter_fn.implicit_filter.{i}.freq"].grad for i in (1, 3, 5)).reshape(-1)
        if key == "dz":
            ref = ref[0, :L]
        assert g[key].shape == ref.shape, (name, g[key].shape, ref.shape)
        rel = ((g[key] - ref).norm() / ref.norm()).item()
        assert rel < 1e-12, (name, rel)


def test_row_pitch_beyond_32_bit_offsets_is_rejected(emu_backend):
    """D * ldk * 4 > 2^31 -- where the kernels' 32-bit byte offsets wrap and their descriptor size truncates -- returns HYENA_ERR_BAD_ARG from all
    four _ld entry points before anything is launched (the buffers here are a few floats)"""
    lib, bf16 = emu_backend.lib(), emu_backend.dtype_code(torch.bfloat16)
    for D, ldk_ok in ((256, 1 << 21), (128, 1 << 22), (64, 1 << 23)):
        args = FLoc.make_case(D, 4, 5, seed=0)
        p = FLoc._params(emu_backend, args, 0.0, True)
        buf = torch.zeros(64)
        g = emu_backend.FilterGrads()
        for n in ("dw0", "db0", "dw1", "db1", "dw2", "db2", "dw3", "dfreq"):
            setattr(g, n, buf.data_ptr())
        nbytes = int(lib.hyena_filter_workspace_bytes(4, D))
        for ldk in (ldk_ok + 1, 1 << 24, (1 << 31) - 1):
            assert lib.hyena_filter_fwd_ld(ctypes.byref(p), buf.data_ptr(), ldk, None, None) == 1
            assert lib.hyena_filter16_fwd_ld(ctypes.byref(p), bf16, buf.data_ptr(), ldk, None, None) == 1
            # (a workspace pointer that is never touched: the call returns on the pitch before it looks at anything else it would use)
            assert lib.hyena_filter_bwd_ld(ctypes.byref(p), buf.data_ptr(), ldk, buf.data_ptr(), ctypes.byref(g), buf.data_ptr(), nbytes, None) == 1
            assert lib.hyena_filter16_bwd_ld(ctypes.byref(p), bf16, buf.data_ptr(), ldk, buf.data_ptr(), ctypes.byref(g), buf.data_ptr(), nbytes, None) == 1
    # the largest pitch a real caller reaches stays accepted: D = 256 rows of HYENA_MAX_L floats (checked by value: nothing is launched here)
    assert 256 * (1 << 20) * 4 <= 1 << 31

"""The pitched entry points at their 32-bit offset limits, on the CPU emulation of the kernels (the same kernel source with the same integer types: an
offset that wraps on the device wraps here).  Cases, layout and references: tests/limits_local.py; the table: profiles/limits_local.md."""
import pytest
import torch

from tests import limits_local as LL

CPU = torch.device("cpu")
TOUCH_CAP = 64 << 20                          # bytes of pages one emulator case may touch in its far-apart tensors


@pytest.mark.parametrize("i", range(len(LL.FFT_CASES)), ids=LL.FFT_IDS)
def test_fftconv_far_apart_rows(emu_backend, monkeypatch, i):
    st, touched = LL.fft_case(emu_backend, CPU, monkeypatch, i, label="emu")
    assert touched <= TOUCH_CAP


def test_inproj_vg_pitch_at_its_limit(emu_backend):
    st, touched = LL.inproj_case(emu_backend, CPU, torch.bfloat16, label="emu")
    assert touched <= TOUCH_CAP


@pytest.mark.parametrize("which", ["lda", "csx"])
def test_cm_rows_across_4_gib(emu_backend, which):
    LL.cm_case(emu_backend, CPU, torch.bfloat16, which, label="emu")


@pytest.mark.parametrize("T", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_filter16_rows_at_the_pitch_limit(emu_backend, T):
    assert LL.filter16_case(emu_backend, CPU, T, label="emu") <= TOUCH_CAP


# ---- the Python layer: limits it can know beforehand never surface as a refusal of the library in the middle of a step -------------------------
class _Plan:
    """the library's answers about a length, stubbed: nothing is loaded or launched"""

    def __init__(self, plan, M):
        self.plan, self.M = plan, M

    def hyena_fftconv_plan(self, L):
        return self.plan

    def hyena_fftconv_fft_size(self, L):
        return self.M


def test_backward_batch_is_cut_at_the_row_offset_limit(monkeypatch):
    from hyena_dna_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: _Plan(_lib.PLAN_ONCHIP, 1024))
    assert _lib.fftconv_bwd_batch(8191, 256, 1024, 1024, 2) == 8191                    # B D ldx es = 2^32 - 2^19: one call
    for B, D, ld, es in ((8192, 256, 1024, 2), (20000, 256, 1024, 2), (4096, 256, 1024, 4), (300, 128, 1 << 16, 4), (140000, 128, 64, 4)):
        nb = _lib.fftconv_bwd_batch(B, D, 5, ld, es)
        assert 1 <= nb < B and nb * D * ld * es < 2 ** 32 <= (nb + 1) * D * ld * es, (B, D, ld, es, nb)
    with pytest.raises(_lib.HyenaLibraryError, match="2\\^32"):
        _lib.fftconv_bwd_batch(2, 256, 1024, 1 << 23, 2)                                 # one item alone is past the limit
    # from M = 2048 on, and on the two-level plan, nothing is cut
    monkeypatch.setattr(_lib, "lib", lambda: _Plan(_lib.PLAN_ONCHIP, 2048))
    assert _lib.fftconv_bwd_batch(1 << 20, 256, 2048, 2048, 2) == 1 << 20
    monkeypatch.setattr(_lib, "lib", lambda: _Plan(_lib.PLAN_TWO_LEVEL, 65536))
    assert _lib.fftconv_bwd_batch(1 << 20, 256, 40000, 40000, 2) == 1 << 20


def test_channels_past_the_spectrum_limit_raise_before_anything_is_allocated(monkeypatch):
    from hyena_dna_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: _Plan(_lib.PLAN_ONCHIP, 32768))
    _lib.fftconv_check_channels(16383, 32768)
    with pytest.raises(_lib.HyenaLibraryError, match="at most 16383 channels"):
        _lib.fftconv_check_channels(16384, 32768)
    monkeypatch.setattr(_lib, "lib", lambda: _Plan(_lib.PLAN_TWO_LEVEL, 65536))
    _lib.fftconv_check_channels(1 << 20, 40000)                                          # the two-level plan works in chunks of channels
    # through the wrappers: tensors without storage, so anything that touched or allocated one would fail differently
    monkeypatch.setattr(_lib, "lib", lambda: _Plan(_lib.PLAN_ONCHIP, 32768))
    monkeypatch.setattr(_lib, "_require_gpu", lambda t, name: None)
    u = torch.empty((1, 16384, 32765), dtype=torch.bfloat16, device="meta")
    k = torch.empty((16384, 32765), device="meta")
    with pytest.raises(_lib.HyenaLibraryError, match="at most 16383 channels"):
        _lib.fftconv_fwd(u, k, None)
    with pytest.raises(_lib.HyenaLibraryError, match="at most 16383 channels"):
        _lib.fftconv_bwd(u, u, k, None)


def test_backward_in_batch_slices_gives_the_whole_batch(emu_backend, monkeypatch):
    """fftconv_bwd's route around the limit, forced at a small shape: du bit for bit the unsliced call's, dk and dbias -- sums in another order --
    within the bounds of tests/fftconv_local.py; a ragged last slice; with the forward's spectrum and without"""
    from tests import fftconv_local as FL
    B, D, L, T = 5, 3, 1021, torch.bfloat16
    u, k, b, dout = FL.inputs(B, D, L, T, 4242)
    ref = FL.ref64(u, k, b, dout)
    for saved in (False, True):
        sp = emu_backend.fftconv_fwd(u, k, b, save=True)[1] if saved else None
        whole = emu_backend.fftconv_bwd(dout, u, k, b, saved=sp)
        calls = []
        real = emu_backend.lib().hyena_fftconv_bwd_ld
        with monkeypatch.context() as m:
            m.setattr(emu_backend, "fftconv_bwd_batch", lambda *a: 2)
            m.setattr(emu_backend.lib(), "hyena_fftconv_bwd_ld", lambda *a: (calls.append(a[7]), real(*a))[1], raising=False)
            du, dk, db = emu_backend.fftconv_bwd(dout, u, k, b, saved=sp)
        assert calls == [2, 2, 1]
        assert FL.same_bits(du, whole[0])
        st = FL.Stats()
        st.hold32("dk", dk, ref[2], FL.c_bound(L)[2])
        assert float((db.double() - ref[3]).abs().max()) < 3e-6 * (B * L) ** 0.5 + 1e-6
        du2, dk2, db2 = emu_backend.fftconv_bwd(dout, u, k, b, need_du=False, saved=sp)
        assert du2 is None and dk2 is not None


def test_filter_rows_at_the_pitch_limit(emu_backend):
    assert LL.filter_case(emu_backend, CPU, label="emu") <= TOUCH_CAP


@pytest.mark.parametrize("which", ["gen1", "gen2", "dgrad"])
def test_outproj_rows_across_4_gib(emu_backend, which):
    LL.outproj_case(emu_backend, CPU, torch.float16 if which == "dgrad" else torch.bfloat16, which, label="emu")


@pytest.mark.parametrize("form", ["single", "rows", "block"])
def test_decode_conv_rows_across_4_gib(emu_backend, form):
    LL.decode_conv_case(emu_backend, CPU, torch.bfloat16, form, label="emu")

"""Edited windows of one reference sequence: the state that carries M windows through the mixers (``EditWindowParams``).

Embedding, LayerNorm, MLP, the gates and the 3-tap short convolution of the HyenaDNA model are per-position or causal, and the long
convolution is LINEAR in its input ``vg = v * x1``.  A sequence that equals the reference below position p therefore has, in every layer
and at every t >= p, the reference's own long-convolution output plus a short causal convolution of the difference of the inputs::

    delta[s] = vg_alt[s] - vg_ref[s]   (0 for s < p)        y_alt[t] = y_ref[t] + sum_{s = p .. t} k[t - s] delta[s] + fb delta[t]

One pass over the reference (the REFERENCE phase) serves every edit; an edit then costs a window of T positions through the per-position
layers plus a T x T triangular Toeplitz product per channel and layer (the WINDOW phase; csrc/variant_kernels.h).  No history is streamed.

``EditWindowParams`` travels where ``InferenceParams`` travels -- ``model(ids, inference_params=ew)`` -- and ``HyenaOperator.forward``
dispatches on its type.  ``HyenaDNALM.forward_edited_windows`` / ``score_variants`` / ``saturation_mutagenesis`` drive it.
"""
import torch

from . import _lib

__all__ = ["EditWindowParams", "EditWindowLayer"]


class EditWindowLayer:
    """what one operator keeps of the reference for M windows of T positions: ``tail`` (3D, M, 2) fp32 raw in_proj outputs at pos - 2, pos - 1;
    ``vg_ref`` (M, D, T) I/O type and ``y_ref`` (M, D, T) fp32, the long convolution's input and output over the windows (zeros past the
    sequence's end); ``k`` (D, T) fp32 and ``fb`` (D,), the filter's first T taps and the convolution bias; the short filter and the in_proj
    bias in fp32, as a decode cache keeps them.  A snapshot of the weights at the reference phase."""
    __slots__ = ("tail", "vg_ref", "y_ref", "k", "fb", "bin", "w", "b")


class EditWindowParams:
    """M windows of ``T`` positions; window m replaces positions ``[positions[m], positions[m] + T)`` of reference row ``groups[m]``.

    ``positions`` (M,) int64 and ``groups`` (M,) int64 on the model's device (``groups=None``: row 0), ``1 <= T <= 1024``.  ``phase``:
    "reference" (the next forward runs the (G, L) reference and keeps every layer's windows in ``layers``), then "window" (every further
    forward takes (m, T) window rows).  ``select(lo, hi)`` restricts the window phase to windows lo ... hi - 1, so that a caller can run
    the windows in chunks.  Windows that run past the sequence's end are clipped: what is kept there is zeros, and the caller drops the rows."""

    def __init__(self, positions, groups, T):
        T = int(T)
        if not 1 <= T <= _lib.VARIANT_TMAX:
            raise ValueError(f"T={T}: an edited window holds 1 ... {_lib.VARIANT_TMAX} positions")
        if not torch.is_tensor(positions) or positions.dim() != 1 or positions.dtype != torch.int64 or positions.shape[0] < 1:
            raise ValueError("positions has to be an (M >= 1,) int64 tensor")
        if groups is None:
            groups = torch.zeros_like(positions)
        if not torch.is_tensor(groups) or groups.shape != positions.shape or groups.dtype != torch.int64 or groups.device != positions.device:
            raise ValueError("groups has to be an int64 tensor of positions' shape on positions' device")
        self.positions, self.groups, self.T = positions, groups, T
        self.pos32 = positions.to(torch.int32).contiguous()
        self.phase = "reference"
        self.layers = {}
        self.L = None
        self.lo, self.hi = 0, positions.shape[0]

    def select(self, lo, hi):
        if not 0 <= lo < hi <= self.positions.shape[0]:
            raise ValueError(f"select({lo}, {hi}): windows 0 ... {self.positions.shape[0]}")
        self.lo, self.hi = int(lo), int(hi)

    def store_reference(self, key, op, xT, vg, k, fb, L):
        """after an operator's reference forward over L positions: xT (3D, G, L) raw in_proj outputs, vg (G, D, L) the long convolution's
        input, k (D, L) and fb (D,) its filter and bias.  The long convolution's own output y_ref comes once from the forward kernels
        (``_lib.fftconv_fwd``) in fp32 -- with a 16-bit I/O type on an fp32 copy of vg, both freed when this returns -- and only the M windows
        of tail, vg_ref and y_ref are kept (plain tensor indexing: one-time, M T D elements)."""
        G, D = vg.shape[0], vg.shape[1]
        dev = vg.device
        if self.positions.device != dev:
            raise ValueError(f"positions live on {self.positions.device}, the model runs on {dev}")
        if self.L is not None and self.L != L:
            raise ValueError(f"the reference phase ran over {self.L} positions in an earlier layer and over {L} here")
        self.L = L
        T = self.T
        M = self.positions.shape[0]
        st = EditWindowLayer()
        idx = self.positions[:, None] + torch.arange(T, device=dev)[None, :]                    # (M, T) absolute positions
        valid = idx < L
        idxc = idx.clamp(0, L - 1)
        g = self.groups
        rows = torch.arange(D, device=dev)
        vg_ref = vg[g[:, None, None], rows[None, :, None], idxc[:, None, :]]                    # (M, D, T)
        st.vg_ref = torch.where(valid[:, None, :], vg_ref, torch.zeros((), dtype=vg.dtype, device=dev)).contiguous()
        tidx = self.positions[:, None] + torch.tensor([-2, -1], device=dev)[None, :]            # (M, 2)
        tail = xT[:, g[:, None], tidx.clamp(0, L - 1)].to(torch.float32)                        # (3D, M, 2)
        st.tail = (tail * ((tidx >= 0) & (tidx < L))[None]).contiguous()
        k32 = k.detach().to(torch.float32)
        fb32 = fb.detach().to(torch.float32).reshape(D)
        if vg.dtype == torch.float32:
            vg32 = vg
        else:
            vg32 = _lib.empty_like_rows(_lib.as_rows(vg), dtype=torch.float32)
            vg32.copy_(vg)
        y = _lib.fftconv_fwd(vg32, k32, fb32, grad=False)                                       # (G, D, L) fp32
        del vg32
        y_ref = y[g[:, None, None], rows[None, :, None], idxc[:, None, :]]
        del y
        st.y_ref = torch.where(valid[:, None, :], y_ref, torch.zeros((), dtype=torch.float32, device=dev)).contiguous()
        st.k = torch.zeros(D, T, dtype=torch.float32, device=dev)
        st.k[:, :min(T, L)].copy_(k32[:, :min(T, L)])
        st.fb = fb32.clone()
        st.bin = op.in_proj.bias.detach().to(torch.float32).clone() if op.in_proj.bias is not None else None
        st.w = op.short_filter.weight.detach().to(torch.float32).reshape(3 * D, 3).clone()
        st.b = op.short_filter.bias.detach().to(torch.float32).clone()
        assert st.vg_ref.shape == (M, D, T)
        self.layers[key] = st

    def step(self, st, x3):
        """x3 (m, T, 3D): in_proj output of the selected windows' rows without bias -> z (m, T, D) for out_proj (two kernels)"""
        lo, hi = self.lo, self.hi
        m, T, D3 = x3.shape
        D = D3 // 3
        if m != hi - lo or T != self.T:
            raise ValueError(f"the window phase takes ({hi - lo}, {self.T}) window rows (got ({m}, {T})): one row per selected window")
        if x3.dtype != st.vg_ref.dtype:
            raise ValueError(f"the window phase runs in {x3.dtype}, the reference phase ran in {st.vg_ref.dtype}")
        whole = lo == 0 and hi == self.positions.shape[0]
        tail = st.tail if whole else st.tail[:, lo:hi].contiguous()
        x0 = torch.empty(m, T, D, dtype=torch.float32, device=x3.device)
        delta = torch.empty(m, D, T, dtype=torch.float32, device=x3.device)
        z = torch.empty(m, T, D, dtype=x3.dtype, device=x3.device)
        _lib.variant_pre(x3.contiguous(), st.bin, st.w, st.b, tail, self.pos32[lo:hi], st.vg_ref[lo:hi], x0, delta)
        _lib.variant_conv(st.y_ref[lo:hi], delta, st.k, st.fb, x0, z)
        return z

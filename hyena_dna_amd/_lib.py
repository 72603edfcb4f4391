"""ctypes binding of the C ABI in include/hyena_fftconv.h (libhyena_fftconv.so, built by hyena_dna_amd.build).

The library is loaded lazily on first use.  There is deliberately no fallback: if the shared object is missing
or a call returns a non-zero status the caller gets an exception, never a silently different code path.
"""
import ctypes
import os
import threading

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libhyena_fftconv.so")
ABI_VERSION = 3

HYENA_F32, HYENA_BF16, HYENA_F16 = 0, 1, 2
MAX_L = 1048576
PLAN_NONE, PLAN_ONCHIP, PLAN_TWO_LEVEL = 0, 1, 2

_DTYPES = {torch.float32: HYENA_F32, torch.bfloat16: HYENA_BF16, torch.float16: HYENA_F16}

_lock = threading.Lock()
_lib = None
_tables = {}      # (device index, M) -> uint8 tensor holding the twiddle tables
_workspace = {}   # (device index, stream) -> uint8 tensor


class HyenaLibraryError(RuntimeError):
    pass


class FilterParams(ctypes.Structure):
    """hyena_filter_params of include/hyena_filter.h."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("z", "t", "w0", "b0", "w1", "b1", "w2", "b2", "w3", "freq", "deltas")] + \
               [("shift", ctypes.c_float), ("modulate", ctypes.c_int), ("z_stride", ctypes.c_int),
                ("L", ctypes.c_int), ("E", ctypes.c_int), ("D", ctypes.c_int)]


class FilterGrads(ctypes.Structure):
    """hyena_filter_grads of include/hyena_filter.h."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("dw0", "db0", "dw1", "db1", "dw2", "db2", "dw3", "dfreq", "dz")]


class _HipBackend:
    """Where tensors live and how the library is reached.  The product has exactly this one backend (ROCm device
    tensors + libhyena_fftconv.so); tests/ substitute a CPU-emulation double to exercise the host logic without
    a GPU (tests/hipemu/emu_backend.py) -- nothing in this package ever selects another backend."""
    name = "hip"
    path = os.environ.get("HYENA_FFTCONV_LIB", LIB_PATH)      # (development: A/B builds of the same HIP library)

    def require(self, t, name):
        if not t.is_cuda:
            raise HyenaLibraryError(
                f"hyena fftconv: `{name}` lives on {t.device}; the HIP kernels need a ROCm device tensor "
                "(there is no CPU fallback)")

    def guard(self, device):
        return torch.cuda.device(device)

    def stream(self, device):
        return torch.cuda.current_stream(device).cuda_stream

    def capturing(self):
        return torch.cuda.is_current_stream_capturing()

    def free_memory(self, device=None):
        """Bytes a new allocation on `device` can take: what the driver reports free plus what PyTorch's caching
        allocator holds but is not using (it hands those blocks out again without asking the driver)."""
        if torch.cuda.is_current_stream_capturing():      # no driver queries inside a hipGraph capture
            return None
        return (torch.cuda.mem_get_info(device)[0] + torch.cuda.memory_reserved(device)
                - torch.cuda.memory_allocated(device))


_backend = _HipBackend()


def lib():
    """The loaded shared library; raises HyenaLibraryError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        LIB_PATH = _backend.path
        if not os.path.exists(LIB_PATH):
            raise HyenaLibraryError(
                f"{LIB_PATH} not found: build it with `python -m hyena_dna_amd.build` (hipcc, gfx950). "
                "hyena_dna_amd has no CPU/PyTorch fallback for the long convolution.")
        L = ctypes.CDLL(LIB_PATH)
        c_int, c_size_t, c_void_p, c_char_p = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p
        L.hyena_fftconv_abi_version.restype = c_int
        L.hyena_fftconv_abi_version.argtypes = []
        L.hyena_fftconv_error_string.restype = c_char_p
        L.hyena_fftconv_error_string.argtypes = [c_int]
        L.hyena_fftconv_fft_size.restype = c_int
        L.hyena_fftconv_fft_size.argtypes = [c_int]
        L.hyena_fftconv_plan.restype = c_int
        L.hyena_fftconv_plan.argtypes = [c_int]
        L.hyena_fftconv_table_bytes.restype = c_size_t
        L.hyena_fftconv_table_bytes.argtypes = [c_int]
        L.hyena_fftconv_init_tables.restype = c_int
        L.hyena_fftconv_init_tables.argtypes = [c_void_p, c_int, c_void_p]
        L.hyena_fftconv_default_chunk.restype = c_int
        L.hyena_fftconv_default_chunk.argtypes = [c_int, c_int, c_int, c_int]
        L.hyena_fftconv_workspace_bytes.restype = c_size_t
        L.hyena_fftconv_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int, c_int]
        L.hyena_fftconv_fwd.restype = c_int
        L.hyena_fftconv_fwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_size_t, c_int, c_void_p]
        L.hyena_fftconv_bwd.restype = c_int
        L.hyena_fftconv_bwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_int, c_void_p]
        L.hyena_fftconv_saved_bytes.restype = c_size_t
        L.hyena_fftconv_saved_bytes.argtypes = [c_int, c_int, c_int]
        L.hyena_fftconv_fwd_save.restype = c_int
        L.hyena_fftconv_fwd_save.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                             c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_void_p]
        L.hyena_fftconv_bwd_saved.restype = c_int
        L.hyena_fftconv_bwd_saved.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                              c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_void_p]
        L.hyena_fftconv_fwd_ld.restype = c_int
        L.hyena_fftconv_fwd_ld.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                           c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_void_p]
        L.hyena_fftconv_bwd_ld.restype = c_int
        L.hyena_fftconv_bwd_ld.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_int,
                                           c_void_p, c_size_t, c_void_p]
        # fused mixer shell (include/hyena_mixer.h)
        L.hyena_mixer_pre_fwd.restype = c_int
        L.hyena_mixer_pre_fwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]
        L.hyena_mixer_post_fwd.restype = c_int
        L.hyena_mixer_post_fwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                           c_void_p]
        L.hyena_mixer_partial_floats.restype = c_size_t
        L.hyena_mixer_partial_floats.argtypes = [c_int, c_int, c_int]
        L.hyena_mixer_post_bwd.restype = c_int
        L.hyena_mixer_post_bwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int, c_int, c_int, c_int, c_int, c_void_p]
        L.hyena_mixer_pre_bwd.restype = c_int
        L.hyena_mixer_pre_bwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_int, c_int, c_int, c_int, c_int, c_void_p]
        # the same shell in channel-major layout (csrc/cm_kernels.h)
        L.hyena_cm_partial_floats.restype = c_size_t
        L.hyena_cm_partial_floats.argtypes = [c_int, c_int, c_int]
        L.hyena_cm_pre_fwd.restype = c_int
        L.hyena_cm_pre_fwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]
        L.hyena_cm_post_fwd.restype = c_int
        L.hyena_cm_post_fwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p]
        L.hyena_cm_post_bwd.restype = c_int
        L.hyena_cm_post_bwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_int, c_int, c_int, c_int, c_int, c_void_p]
        L.hyena_cm_pre_bwd.restype = c_int
        L.hyena_cm_pre_bwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int, c_int, c_int, c_int, c_int, c_void_p]
        L.hyena_cm_pre_fwd_ld.restype = c_int
        L.hyena_cm_pre_fwd_ld.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, ctypes.c_long, c_int, c_int,
                                          c_int, c_void_p]
        L.hyena_cm_post_fwd_ld.restype = c_int
        L.hyena_cm_post_fwd_ld.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, ctypes.c_long, c_int,
                                           ctypes.c_long, c_int, c_int, c_int, c_void_p]
        L.hyena_cm_post_bwd_ld.restype = c_int
        L.hyena_cm_post_bwd_ld.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int, c_int, c_int, c_int, ctypes.c_long, c_int, ctypes.c_long, c_int, c_int, c_int, c_void_p]
        L.hyena_cm_pre_bwd_ld.restype = c_int
        L.hyena_cm_pre_bwd_ld.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_int, c_int, c_int, c_int, ctypes.c_long, c_int, c_int, c_int, c_void_p]
        # one-position decode step (include/hyena_decode.h)
        L.hyena_decode_partial_floats.restype = c_size_t
        L.hyena_decode_partial_floats.argtypes = [c_int, c_int, c_int]
        L.hyena_decode_pre.restype = c_int
        L.hyena_decode_pre.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]
        L.hyena_decode_conv.restype = c_int
        L.hyena_decode_conv.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]
        L.hyena_decode_post.restype = c_int
        L.hyena_decode_post.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]
        for rows, one in ((L.hyena_decode_pre_rows, L.hyena_decode_pre), (L.hyena_decode_conv_rows, L.hyena_decode_conv),
                          (L.hyena_decode_post_rows, L.hyena_decode_post)):          # per-row positions: same arguments, pos -> B ints
            rows.restype, rows.argtypes = c_int, one.argtypes
        # fan-out: B = G fan rows, history columns [0, S) once per group, [S, Lcap) per row
        L.hyena_decode_pre_fan.restype = c_int
        L.hyena_decode_pre_fan.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]
        L.hyena_decode_conv_fan.restype = c_int
        L.hyena_decode_conv_fan.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                            c_int, c_int, c_void_p]
        L.hyena_decode_post_fan.restype = c_int
        L.hyena_decode_post_fan.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                            c_int, c_void_p]
        # block step: T positions per call -- the arguments of the single-position / fan call with T before dtype
        L.hyena_decode_block_partial_floats.restype = c_size_t
        L.hyena_decode_block_partial_floats.argtypes = [c_int, c_int, c_int, c_int]
        for blk, one in ((L.hyena_decode_pre_block, L.hyena_decode_pre), (L.hyena_decode_conv_block, L.hyena_decode_conv),
                         (L.hyena_decode_post_block, L.hyena_decode_post), (L.hyena_decode_pre_block_fan, L.hyena_decode_pre_fan),
                         (L.hyena_decode_conv_block_fan, L.hyena_decode_conv_fan), (L.hyena_decode_post_block_fan, L.hyena_decode_post_fan)):
            blk.restype, blk.argtypes = c_int, one.argtypes[:-1] + [c_int, c_void_p]
        # lookahead carry: the history's share of the next W outputs, and the step on [base, t]
        L.hyena_decode_carry_partial_floats.restype = c_size_t
        L.hyena_decode_carry_partial_floats.argtypes = [c_int, c_int, c_int, c_int]
        L.hyena_decode_carry.restype = c_int
        L.hyena_decode_carry.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                         c_int, c_void_p]
        L.hyena_decode_conv_la.restype = c_int
        L.hyena_decode_conv_la.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                           c_void_p]
        L.hyena_decode_post_la.restype = c_int
        L.hyena_decode_post_la.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                           c_int, c_int, c_int, c_void_p]
        # edited windows of a reference sequence (include/hyena_variant.h)
        L.hyena_variant_pre.restype = c_int
        L.hyena_variant_pre.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_int, c_int, c_int, c_int, c_void_p]
        L.hyena_variant_conv.restype = c_int
        L.hyena_variant_conv.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]
        L.hyena_decode_sample.restype = c_int
        L.hyena_decode_sample.argtypes = [c_void_p, ctypes.c_long, c_int, c_int, c_int, c_int, ctypes.c_float, c_int, ctypes.c_float, c_void_p,
                                          c_int, c_int, c_void_p, c_void_p, c_void_p, ctypes.c_long, c_int, c_void_p, ctypes.c_long,
                                          c_void_p, c_void_p, c_void_p]
        L.hyena_decode_sample_constrained.restype = c_int
        L.hyena_decode_sample_constrained.argtypes = L.hyena_decode_sample.argtypes[:-1] + [c_void_p, ctypes.c_long, c_int, c_void_p, c_void_p,
                                                                                           ctypes.c_long, c_void_p]
        # beam search: the beam step, the fan-out cache's re-parenting, the backtrack
        L.hyena_decode_beam.restype = c_int
        L.hyena_decode_beam.argtypes = [c_void_p, ctypes.c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, ctypes.c_long, c_int, c_void_p, ctypes.c_long, c_int, c_void_p, c_void_p,
                                        c_void_p, ctypes.c_long, c_int, c_void_p]
        L.hyena_decode_reorder_fan.restype = c_int
        L.hyena_decode_reorder_fan.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                               c_int, c_void_p]
        L.hyena_decode_beam_backtrack.restype = c_int
        L.hyena_decode_beam_backtrack.argtypes = [c_void_p, c_void_p, c_void_p, ctypes.c_long, c_int, c_int, c_int, c_int, c_void_p,
                                                  ctypes.c_long, c_int, c_void_p, ctypes.c_long, c_void_p]
        # automaton-constrained generation: the sampler and the beam step with the mask from (state, new-token number) tables
        auto_args = [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]              # M, Nt, S, delta, Vdelta, dstate
        L.hyena_decode_sample_automaton.restype = c_int
        L.hyena_decode_sample_automaton.argtypes = L.hyena_decode_sample.argtypes[:-1] + auto_args + [c_void_p, c_void_p, ctypes.c_long, c_void_p]
        L.hyena_decode_beam_automaton.restype = c_int
        L.hyena_decode_beam_automaton.argtypes = L.hyena_decode_beam.argtypes[:17] + auto_args + L.hyena_decode_beam.argtypes[20:]
        # input projection on the matrix cores + front of the shell (include/hyena_proj.h)
        L.hyena_inproj_pre_fwd_ld.restype = c_int
        L.hyena_inproj_pre_fwd_ld.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_int, c_int, c_int, c_int, ctypes.c_long, c_int, c_int, c_int, c_void_p]
        L.hyena_outproj_gate_addnorm_fwd_ld.restype = c_int
        L.hyena_outproj_gate_addnorm_fwd_ld.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                        c_void_p, ctypes.c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                        c_int, c_int, c_int, c_int, ctypes.c_long, c_int, ctypes.c_long, c_int, c_int, c_int,
                                                        c_void_p]
        L.hyena_outproj_dgrad_supported.restype = c_int
        L.hyena_outproj_dgrad_supported.argtypes = [c_int, c_int, c_int, c_int]
        L.hyena_outproj_dgrad_partial_floats.restype = c_size_t
        L.hyena_outproj_dgrad_partial_floats.argtypes = [c_int, c_int, c_int]
        L.hyena_outproj_dgrad_gate_bwd_ld.restype = c_int
        L.hyena_outproj_dgrad_gate_bwd_ld.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                      c_void_p, c_int, c_int, c_int, c_int, ctypes.c_long, c_int, c_int, c_int, c_void_p]
        L.hyena_outproj_gate_fwd_ld.restype = c_int
        L.hyena_outproj_gate_fwd_ld.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_int, c_int, c_int, c_int, ctypes.c_long, c_int, ctypes.c_long, c_int, c_int, c_int, c_void_p]
        L.hyena_proj_supported.restype = c_int
        L.hyena_proj_supported.argtypes = [c_int, c_int, c_int, c_int]
        L.hyena_inproj_pre_fwd.restype = c_int
        L.hyena_inproj_pre_fwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int, c_int, c_int, c_int, c_int, c_void_p]
        L.hyena_outproj_supported.restype = c_int
        L.hyena_outproj_supported.argtypes = [c_int, c_int, c_int, c_int]
        L.hyena_proj_kernel_generation.restype = c_int
        L.hyena_proj_kernel_generation.argtypes = [c_int, c_int]
        gen = os.environ.get("HYENA_OUTPROJ_KERNEL")              # A/B knob: 1 = round 4's out_proj kernel, 2 (default) = round 6's
        if gen in ("1", "2"):
            L.hyena_proj_kernel_generation(0, int(gen))
        gen = os.environ.get("HYENA_INPROJ_KERNEL")               # A/B knob: 1 (default) = rounds 3 / 4's in_proj kernel, 2 = round 6's (not faster: see the header)
        if gen in ("1", "2"):
            L.hyena_proj_kernel_generation(1, int(gen))
        L.hyena_outproj_gate_fwd.restype = c_int
        L.hyena_outproj_gate_fwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_int, c_int, c_int, c_int, c_int, c_void_p]
        L.hyena_colsum_supported.restype = c_int
        L.hyena_colsum_supported.argtypes = [ctypes.c_long, c_int, c_int]
        L.hyena_colsum_partial_floats.restype = c_size_t
        L.hyena_colsum_partial_floats.argtypes = [ctypes.c_long, c_int]
        L.hyena_colsum.restype = c_int
        L.hyena_colsum.argtypes = [c_void_p, c_void_p, c_void_p, ctypes.c_long, c_int, c_int, c_void_p]
        L.hyena_mlp_supported.restype = c_int
        L.hyena_mlp_supported.argtypes = [ctypes.c_long, c_int, c_int, c_int]
        L.hyena_mlp_partial_floats.restype = c_size_t
        L.hyena_mlp_partial_floats.argtypes = [ctypes.c_long, c_int]
        L.hyena_mlp_fc1_gelu_fwd.restype = c_int
        L.hyena_mlp_fc1_gelu_fwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_long, c_int, c_int, c_int, c_void_p]
        L.hyena_mlp_dh_dgelu_bwd.restype = c_int
        L.hyena_mlp_dh_dgelu_bwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_long, c_int, c_int, c_int, c_void_p]
        # fused implicit filter (include/hyena_filter.h)
        L.hyena_filter_supported.restype = c_int
        L.hyena_filter_supported.argtypes = [c_int, c_int, c_int, c_int]
        L.hyena_filter_saved_bytes.restype = c_size_t
        L.hyena_filter_saved_bytes.argtypes = [c_int]
        L.hyena_filter_workspace_bytes.restype = c_size_t
        L.hyena_filter_workspace_bytes.argtypes = [c_int, c_int]
        L.hyena_filter_fwd.restype = c_int
        L.hyena_filter_fwd.argtypes = [ctypes.POINTER(FilterParams), c_void_p, c_void_p, c_void_p]
        L.hyena_filter_bwd.restype = c_int
        L.hyena_filter_bwd.argtypes = [ctypes.POINTER(FilterParams), c_void_p, c_void_p, ctypes.POINTER(FilterGrads),
                                       c_void_p, c_size_t, c_void_p]
        L.hyena_filter16_saved_bytes.restype = c_size_t
        L.hyena_filter16_saved_bytes.argtypes = [c_int]
        L.hyena_filter16_fwd.restype = c_int
        L.hyena_filter16_fwd.argtypes = [ctypes.POINTER(FilterParams), c_int, c_void_p, c_void_p, c_void_p]
        L.hyena_filter16_bwd.restype = c_int
        L.hyena_filter16_bwd.argtypes = [ctypes.POINTER(FilterParams), c_int, c_void_p, c_void_p, ctypes.POINTER(FilterGrads),
                                         c_void_p, c_size_t, c_void_p]
        L.hyena_filter_row_pitch.restype = c_int
        L.hyena_filter_row_pitch.argtypes = [c_int]
        L.hyena_filter_fwd_ld.restype = c_int
        L.hyena_filter_fwd_ld.argtypes = [ctypes.POINTER(FilterParams), c_void_p, c_int, c_void_p, c_void_p]
        L.hyena_filter_bwd_ld.restype = c_int
        L.hyena_filter_bwd_ld.argtypes = [ctypes.POINTER(FilterParams), c_void_p, c_int, c_void_p, ctypes.POINTER(FilterGrads),
                                          c_void_p, c_size_t, c_void_p]
        L.hyena_filter16_fwd_ld.restype = c_int
        L.hyena_filter16_fwd_ld.argtypes = [ctypes.POINTER(FilterParams), c_int, c_void_p, c_int, c_void_p, c_void_p]
        L.hyena_filter16_bwd_ld.restype = c_int
        L.hyena_filter16_bwd_ld.argtypes = [ctypes.POINTER(FilterParams), c_int, c_void_p, c_int, c_void_p, ctypes.POINTER(FilterGrads),
                                            c_void_p, c_size_t, c_void_p]
        # fused residual add + LayerNorm (include/hyena_block.h)
        c_long, c_float = ctypes.c_long, ctypes.c_float
        L.hyena_add_norm_supported.restype = c_int
        L.hyena_add_norm_supported.argtypes = [c_int, c_int, c_int]
        L.hyena_add_norm_fwd.restype = c_int
        L.hyena_add_norm_fwd.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_void_p,
                                         c_void_p, c_void_p, c_long, c_int, c_void_p]
        L.hyena_dropout_add_norm_fwd.restype = c_int
        L.hyena_dropout_add_norm_fwd.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_int,
                                                 c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p]
        L.hyena_dropout_add_norm_bwd.restype = c_int
        L.hyena_dropout_add_norm_bwd.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p,
                                                 c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p]
        L.hyena_dropout_add_norm_bwd_colsum.restype = c_int
        L.hyena_dropout_add_norm_bwd_colsum.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p,
                                                        c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p]
        L.hyena_embed_add_norm_supported.restype = c_int
        L.hyena_embed_add_norm_supported.argtypes = [c_int, c_int, c_int]
        L.hyena_embed_add_norm_fwd.restype = c_int
        L.hyena_embed_add_norm_fwd.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_int,
                                               c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p]
        L.hyena_embed_add_norm_partial_floats.restype = c_size_t
        L.hyena_embed_add_norm_partial_floats.argtypes = [c_long, c_int]
        L.hyena_embed_add_norm_bwd.restype = c_int
        L.hyena_embed_add_norm_bwd.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p,
                                               c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p]
        L.hyena_soft_embed_add_norm_supported.restype = c_int
        L.hyena_soft_embed_add_norm_supported.argtypes = [c_int, c_int, c_int]
        L.hyena_soft_embed_add_norm_fwd.restype = c_int
        L.hyena_soft_embed_add_norm_fwd.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                                    c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_long, c_long, c_int,
                                                    c_void_p]
        L.hyena_soft_embed_add_norm_bwd.restype = c_int
        L.hyena_soft_embed_add_norm_bwd.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p,
                                                    c_float, c_void_p, c_void_p, c_int, c_long, c_long, c_int, c_void_p]
        L.hyena_row_head_supported.restype = c_int
        L.hyena_row_head_supported.argtypes = [c_int, c_int, c_int]
        L.hyena_row_head_fwd.restype = c_int
        L.hyena_row_head_fwd.argtypes = [c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_void_p]
        L.hyena_row_head_bwd.restype = c_int
        L.hyena_row_head_bwd.argtypes = [c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_void_p]
        L.hyena_add_norm_partial_floats.restype = c_size_t
        L.hyena_add_norm_partial_floats.argtypes = [c_long, c_int]
        L.hyena_add_norm_bwd.restype = c_int
        L.hyena_add_norm_bwd.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p]
        L.hyena_add_norm_pool_supported.restype = c_int
        L.hyena_add_norm_pool_supported.argtypes = [c_int, c_int]
        L.hyena_add_norm_pool_partial_floats.restype = c_size_t
        L.hyena_add_norm_pool_partial_floats.argtypes = [c_int, c_long, c_int]
        L.hyena_add_norm_pool_fwd.restype = c_int
        L.hyena_add_norm_pool_fwd.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_int,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long, c_int, c_void_p]
        L.hyena_add_norm_pool_bwd.restype = c_int
        L.hyena_add_norm_pool_bwd.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                              c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long, c_int,
                                              c_void_p]
        if L.hyena_fftconv_abi_version() != ABI_VERSION:
            raise HyenaLibraryError(f"{LIB_PATH}: ABI version {L.hyena_fftconv_abi_version()} != {ABI_VERSION}; rebuild")
        _lib = L
    return _lib


def check(status):
    if status != 0:
        raise HyenaLibraryError("hyena_fftconv: " + lib().hyena_fftconv_error_string(status).decode())


def dtype_code(dtype):
    try:
        return _DTYPES[dtype]
    except KeyError:
        raise TypeError(f"hyena fftconv supports float32 / bfloat16 / float16 activations, got {dtype}") from None


def _require_gpu(t, name):
    _backend.require(t, name)


# ---- pitched rows (round 5) ---------------------------------------------------------------------------------------------------------
# The reference's trainer hands the operator L = max_length - 1 positions (hg38_dataset.py:220-223): odd.  In a packed channel-major tensor
# every second row of 16-bit elements then starts 2 bytes off a 4-byte boundary and none but the first is 16-byte aligned, which the
# kernels' 16-byte accesses, the library GEMMs' vector loads and the filter kernels' fast paths all pay for (21 % of a layer at 2^20 - 1,
# profiles/r5a_*).  So every tensor this package allocates BETWEEN the two projections -- xT, vg, y, zT, their gradients, the filter k and
# dk -- is a [..., :L] view of a buffer whose rows are ROW_ALIGN elements apart (L rounded up): rows start 128-byte (16-bit) / 256-byte
# (fp32) aligned whatever L is, and the C ABI's *_ld entry points are told the pitch.  With L a multiple of ROW_ALIGN nothing changes.
ROW_ALIGN = 64


def row_pitch(L):
    return (int(L) + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN


def empty_rows(lead, L, dtype, device, pitch=None):
    """An uninitialised tensor of shape (*lead, L) whose rows are `pitch` (default row_pitch(L)) elements apart: the [..., :L] view of a
    packed (*lead, pitch) buffer."""
    ld = row_pitch(L) if pitch is None else int(pitch)
    buf = torch.empty(tuple(lead) + (ld,), dtype=dtype, device=device)
    return buf if ld == L else buf[..., :L]


def ld_of(t):
    """Row pitch (elements) of a tensor whose last dimension is contiguous and whose leading dimensions are packed over equally pitched
    rows -- what empty_rows hands out, and every contiguous tensor (pitch = L); None for any other layout."""
    if t.dim() < 1:
        return None
    L = t.shape[-1]
    if L > 1 and t.stride(-1) != 1:
        return None
    if t.dim() == 1:
        return L
    # the pitch is the stride of the innermost leading dimension with more than one entry; all others must be packed over it
    ld, expect = None, None
    for i in range(t.dim() - 2, -1, -1):
        if t.shape[i] == 1:
            continue
        if ld is None:
            ld = t.stride(i)
            if ld < L:
                return None
            expect = ld * t.shape[i]
        else:
            if t.stride(i) != expect:
                return None
            expect *= t.shape[i]
    return L if ld is None else ld


def as_rows(t):
    """t itself if its layout is pitched rows (ld_of), else a packed copy.  A pitched view of ODD length must also own one element behind its last row:
    on pitched rows the two-level plan takes a row's last sample with its regular pair load (csrc/fftconv_kernels.h, tail_pair) and drops the element
    behind it by a select -- that element has to be readable (a caller's view such as buf[..., 1:] of a (B, D, L + 1) tensor ends exactly
    at its storage's end; empty_rows' buffers never do)."""
    ld = ld_of(t)
    if ld is None:
        return t.contiguous()
    L = t.shape[-1] if t.dim() else 0
    if t.dim() >= 2 and ld > L and (L & 1) and t.numel() > 0:
        rows = t.numel() // L
        last = t.storage_offset() + (rows - 1) * ld + L              # first element behind the last row
        if last >= t.untyped_storage().nbytes() // t.element_size():
            return t.contiguous()
    return t


def empty_like_rows(t, dtype=None):
    """A new tensor with t's shape and t's row pitch"""
    return empty_rows(t.shape[:-1], t.shape[-1], t.dtype if dtype is None else dtype, t.device, pitch=ld_of(t))


# Channel-major (C, B, L) tensors that a library GEMM touches as well -- xT, dxT, zT, dzT -- come in a second layout when B > 1: the CHANNEL rows
# are pitched over the flattened positions (row (c, b) at c cs + b L with cs = B L rounded up), so that the GEMM still sees ONE (C, B L) matrix
# with a leading dimension (per-sequence pitched rows would need one product per sequence: 32767 x 8 ran 64 % slower that way,
# profiles/r5h_*) and the in_proj kernel's 64-position tiles over the flattened positions store aligned.  For B = 1 the two layouts coincide.
def empty_cm(C, B, L, dtype, device):
    """uninitialised (C, B, L), channel rows row_pitch(B L) elements apart: strides (cs, L, 1)"""
    cs = row_pitch(B * L)
    buf = torch.empty((C, cs), dtype=dtype, device=device)
    return buf[:, :B * L].view(C, B, L) if B * L > 0 else buf[:, :0].view(C, B, L)


def cm_strides(t):
    """(cs, bs) of a channel-major (C, B, L) tensor -- row (c, b) at element c cs + b bs, rows not overlapping -- or None"""
    if t.dim() != 3:
        return None
    C, B, L = t.shape
    if L > 1 and t.stride(2) != 1:
        return None
    bs = t.stride(1) if B > 1 else L
    if bs < L:
        return None
    need = (B - 1) * bs + L
    cs = t.stride(0) if C > 1 else need
    return (cs, bs) if cs >= need else None


def as_cm(t):
    return t if cm_strides(t) is not None else t.contiguous()


def empty_like_cm(t):
    """a new tensor with t's shape and t's (cs, bs) layout"""
    C, B, L = t.shape
    cs, bs = cm_strides(t)
    buf = torch.empty(max(C * cs, 1), dtype=t.dtype, device=t.device)
    return torch.as_strided(buf, (C, B, L), (cs, bs, 1))


def cm_matrix(t):
    """the (C, B L) matrix view of a channel-major tensor whose sequences follow one another inside a channel row (bs = L), else None"""
    C, B, L = t.shape
    cs, bs = cm_strides(t)
    if B > 1 and bs != L:
        return None
    return torch.as_strided(t, (C, B * L), (cs, 1))


def tables_for(device, L):
    """Twiddle tables for sequence length L on `device` (cached per transform size)."""
    M = lib().hyena_fftconv_fft_size(int(L))
    if M == 0:
        raise HyenaLibraryError(f"hyena fftconv: unsupported sequence length L={L} (1 <= L <= {MAX_L})")
    key = (device.index, M, lib().hyena_fftconv_plan(int(L)))
    t = _tables.get(key)
    if t is None:
        with _lock:
            t = _tables.get(key)
            if t is None:
                nbytes = lib().hyena_fftconv_table_bytes(int(L))
                t = torch.empty(nbytes, dtype=torch.uint8, device=device)
                with _backend.guard(device):
                    check(lib().hyena_fftconv_init_tables(t.data_ptr(), int(L), _backend.stream(device)))
                _tables[key] = t
    return t


_retired = []     # (key, buffer): outgrown workspaces a captured hipGraph of that (device, stream) may still replay on: kept alive
_captured = set() # (device index, stream) keys whose workspace was handed out during a hipGraph capture


def workspace_for(device, nbytes):
    """A per-(device, stream) scratch buffer, grown on demand (geometrically) and reused across calls.  An outgrown buffer
    is freed (stream-ordered, through the caching allocator) unless launches captured into a hipGraph point at it -- only
    then is it retired instead, for the life of the process."""
    stream = _backend.stream(device)
    key = (device.index, stream)
    w = _workspace.get(key)
    capturing = getattr(_backend, "capturing", lambda: False)()
    if w is None or w.numel() < nbytes:
        if w is not None:
            if key in _captured:
                _retired.append((key, w))
                _captured.discard(key)
            nbytes = max(int(nbytes), int(1.5 * w.numel()))
        w = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _workspace[key] = w
    if capturing:
        _captured.add(key)
    return w, stream


def release_stream_state(device, stream):
    """Drop what this module keeps for one (device, stream): its workspace, the record that captured launches point at it, and any
    outgrown buffers retired on its behalf.  Called by the owner of a hipGraph when the graph is released (GraphedTrainStep.release(),
    a sequence-length stage re-capturing): without it every discarded capture stream leaks one workspace."""
    key = (getattr(device, "index", None), stream)
    w = _workspace.pop(key, None)
    _captured.discard(key)
    n = len(_retired)
    _retired[:] = [(k, r) for (k, r) in _retired if k != key]          # the graphs that could replay on them are gone with the stream
    return w is not None or len(_retired) != n


def reset_save_decisions(device=None):
    """Forget the cached keep-the-spectra decisions (all, or one device's): they are taken against the memory that was free when a shape
    was first seen -- re-evaluate them once model + optimizer state exist, at a new GraphedTrainStep, or at a new sequence-length stage."""
    if device is None:
        _save_decision.clear()
        return
    idx = getattr(device, "index", None)
    for key in [k for k in _save_decision if k[0] == idx]:
        del _save_decision[key]


def _chunk_override():
    v = os.environ.get("HYENA_FFTCONV_CHUNK")
    return int(v) if v else 0


def saved_bytes(B, D, L):
    """Size of the optional saved-spectrum buffer (column-transformed filter + activations) for (B, D, L)."""
    return int(lib().hyena_fftconv_saved_bytes(int(B), int(D), int(L)))


_save_decision = {}   # (device index, B, D, L) -> bool


def save_spectra_default(B, D, L, device=None):
    """Keep the forward's column spectra for the backward?  HYENA_FFTCONV_SAVE_SPECTRA = 0 | 1 | auto (default:
    on while the buffer stays below HYENA_FFTCONV_SAVE_LIMIT_GB, default 6 GiB per call)."""
    mode = os.environ.get("HYENA_FFTCONV_SAVE_SPECTRA", "auto").lower()
    if mode in ("0", "off", "false"):
        return False
    if lib().hyena_fftconv_plan(int(L)) == PLAN_ONCHIP:
        # the only intermediate is the filter spectrum H [D][M]: small, and keeping it saves the backward one launch
        # (one transform per channel) -- worth it whenever there is a batch to amortise it over
        return B >= 2 and saved_bytes(B, D, L) <= 256 * 2 ** 20
    if mode in ("1", "on", "true"):
        return True
    need = saved_bytes(B, D, L)
    if need > float(os.environ.get("HYENA_FFTCONV_SAVE_LIMIT_GB", "6")) * 2 ** 30:
        return False
    # per call = per layer: never take more than a quarter of what the device can still give (the recomputing backward
    # fits where this buffer would not).  Decided ONCE per (device, B, D, L): the answer must not flip between steps, nor
    # between an eager warm-up and the hipGraph capture that follows it, with the state of the allocator's cache.
    key = (getattr(device, "index", None), int(B), int(D), int(L))
    hit = _save_decision.get(key)
    if hit is None:
        free = _backend.free_memory(device) if device is not None else _backend.free_memory()
        if free is None:                         # capturing and never decided eagerly: keep the spectra, do not cache
            return True
        hit = _save_decision[key] = bool(need <= free // 4)
    return hit


def fftconv_fwd_keep(u, k, bias, want_grad, keep=None):
    """The forward convolution of an autograd forward -> (out, spectra or None).  What it keeps for the backward -- the column spectra when any
    gradient is wanted and save_spectra_default agrees (time-for-memory trade), otherwise nothing: the backward then recomputes them from
    (u, k) -- is decided here for every caller.  keep: the decision, where it has been taken already (a chain of convolutions of one shape
    takes it once)."""
    if keep is None:
        keep = want_grad and save_spectra_default(*u.shape, device=u.device)
    if keep:
        return fftconv_fwd(u, k, bias, save=True)
    return fftconv_fwd(u, k, bias, grad=want_grad), None


def spectra_hold_input(L):
    """Do the spectra fftconv_fwd(save=True) keeps at this length hold the transform of the convolution's input?  The two-level plan's do; the
    on-chip plan (L <= 32768) keeps the filter's spectrum alone."""
    return lib().hyena_fftconv_plan(int(L)) != PLAN_ONCHIP


def bwd_needs_input(spectra, L):
    """Does fftconv_bwd(..., saved=spectra) read the convolution's input u again (so that a caller who did not keep it has to recompute it)?"""
    return spectra is None or not spectra_hold_input(L)


# ---- the 32-bit offset limits of the workspace-free plan (L <= 32768) that shapes of this package reach (profiles/limits_local.md) ------------
# Both are known from the shape alone, so neither may surface as a refusal of the library in the middle of a step.
def _onchip_r(L):
    """R = M / 1024 of the workspace-free plan, 0 on the two-level plan"""
    return lib().hyena_fftconv_fft_size(int(L)) // 1024 if lib().hyena_fftconv_plan(int(L)) == PLAN_ONCHIP else 0


def fftconv_check_channels(D, L):
    """The on-chip kernels address the filter spectrum H [D][M] through one buffer descriptor with 32-bit byte offsets: D M 8 < 2^32.  Raises --
    before anything is allocated -- where the library would refuse."""
    if D * 1024 * 8 < 2 ** 32 // 32:               # below the limit at every M <= 32768: the common case asks the library nothing
        return
    R = _onchip_r(L)
    if R and D * 1024 * R * 8 >= 2 ** 32:
        raise HyenaLibraryError(f"hyena fftconv: {D} channels at L = {L} put the filter spectrum (D x {1024 * R} x 8 bytes) past the 2^32-byte reach "
                                f"of the on-chip kernels' buffer offsets (L <= 32768): at most {(2 ** 32 - 1) // (1024 * R * 8)} channels per call")


def fftconv_bwd_batch(B, D, L, ldx, es):
    """Batch items one backward call may take.  At L <= 1024 (M = 1024: 32-thread row groups, two to a wavefront) the backward kernels address
    dout / u / du through ONE descriptor over the whole tensor with 32-bit byte offsets, B D ldx es < 2^32, and the library refuses anything
    larger (B = 8192 at D = 256, L = 1024, 16-bit).  fftconv_bwd cuts such a batch into slices of this many items -- du is per item; dk and dbias
    are sums over the batch, added slice by slice."""
    if B * D * ldx * es < 2 ** 32 or _onchip_r(L) != 1:
        return B
    nb = (2 ** 32 - 1) // (D * ldx * es)
    if nb < 1:
        raise HyenaLibraryError(f"hyena fftconv backward: one batch item of {D} channels at row pitch {ldx} ({D * ldx * es} bytes) is past the "
                                f"2^32-byte reach of the 32-bit row offsets at L <= 1024 (L = {L})")
    return nb


def fftconv_fwd(u, k, bias, chunk=None, save=False, grad=None):
    """u (B, D, L), k (D, L) fp32, bias (D,) fp32 or None -> out like u.  u and k may be packed or pitched rows (ld_of); out gets u's pitch.
    save=True additionally returns the saved-spectrum buffer for fftconv_bwd(..., saved=).
    grad: a backward of the same shape will follow (default: save or autograd's grad mode) -- the workspace is then sized
    for it right away instead of being outgrown at the first backward."""
    _require_gpu(u, "u")
    B, D, L = u.shape
    fftconv_check_channels(D, L)
    u, k = as_rows(u), as_rows(k)
    ldx, ldk = ld_of(u), ld_of(k)
    out = empty_like_rows(u)
    if B == 0:                                   # empty batch: nothing to launch (torch.fft returns an empty tensor too)
        return (out, torch.empty(0, dtype=torch.uint8, device=u.device)) if save else out
    chunk = _chunk_override() if chunk is None else int(chunk)
    tables = tables_for(u.device, L)
    nbytes = lib().hyena_fftconv_workspace_bytes(B, D, L, 0, chunk)
    if (save or torch.is_grad_enabled()) if grad is None else grad:
        # a backward of the same shape follows and needs the larger buffer: take it now instead of outgrowing this one
        nbytes = max(nbytes, lib().hyena_fftconv_workspace_bytes(B, D, L, 1, chunk))
    ws, stream = workspace_for(u.device, nbytes)
    bp = bias.data_ptr() if bias is not None else None
    with _backend.guard(u.device):
        saved = torch.empty(saved_bytes(B, D, L), dtype=torch.uint8, device=u.device) if save else None
        check(lib().hyena_fftconv_fwd_ld(u.data_ptr(), k.data_ptr(), bp, out.data_ptr(), B, D, L, ldx, ldk, dtype_code(u.dtype),
                                         tables.data_ptr(), ws.data_ptr(), ws.numel(), chunk,
                                         saved.data_ptr() if save else None, saved.numel() if save else 0, stream))
    return (out, saved) if save else out


def _same_pitch(t, ld):
    """t with row pitch ld (a copy if it has another one)"""
    if ld_of(t) == ld:
        return t
    r = empty_rows(t.shape[:-1], t.shape[-1], t.dtype, t.device, pitch=ld)
    r.copy_(t)
    return r


def fftconv_bwd(dout, u, k, bias, need_du=True, need_dk=True, chunk=None, saved=None):
    """Returns (du like dout | None, dk (D, L) fp32 | None, dbias (D,) fp32 | None).  Packed or pitched rows as in fftconv_fwd: du gets
    dout's pitch, dk gets k's (row_pitch(L) when k is not given).
    With saved= (from fftconv_fwd(save=True)) k is not read, and u only on the workspace-free path (L <= 32768, where
    the saved buffer holds the filter spectrum alone)."""
    _require_gpu(dout, "dout")
    B, D, L = dout.shape
    fftconv_check_channels(D, L)
    dout = as_rows(dout)
    ldx = ld_of(dout)
    nb = fftconv_bwd_batch(B, D, L, ldx, dout.element_size()) if B else 0
    if u is not None:
        u = _same_pitch(as_rows(u), ldx)
    if k is not None:
        k = as_rows(k)
    ldk = ld_of(k) if k is not None else row_pitch(L)
    du = empty_like_rows(dout) if need_du else None
    dk = empty_rows((D,), L, torch.float32, dout.device, pitch=ldk) if need_dk else None
    dbias = torch.empty((D,), dtype=torch.float32, device=dout.device) if need_dk else None
    if B == 0:                                   # empty batch: the parameter gradients are sums over nothing
        return du, None if dk is None else dk.zero_(), None if dbias is None else dbias.zero_()
    chunk = _chunk_override() if chunk is None else int(chunk)
    tables = tables_for(dout.device, L)
    # (a sliced batch: the workspace of its slices -- nb items, and the shorter last one, whose dk may be cut into another number of partial rows)
    nbytes = max(lib().hyena_fftconv_workspace_bytes(b, D, L, 1, chunk) for b in ({B} if nb >= B else {nb, B % nb or nb}))
    ws, stream = workspace_for(dout.device, nbytes)
    bp = bias.data_ptr() if bias is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    with _backend.guard(dout.device):
        # (with the forward's spectra the library reads neither k nor -- for L > 32768 -- u; k is passed only without them)
        if nb >= B:
            check(lib().hyena_fftconv_bwd_ld(dout.data_ptr(), ptr(u), None if saved is not None else ptr(k), bp, ptr(du), ptr(dk), ptr(dbias),
                                             B, D, L, ldx, ldk, dtype_code(dout.dtype), tables.data_ptr(), ws.data_ptr(), ws.numel(),
                                             chunk, ptr(saved), saved.numel() if saved is not None else 0, stream))
            return du, dk, dbias
        # the batch in slices that stay inside the kernels' 32-bit row offsets (fftconv_bwd_batch): the saved buffer of this plan holds the filter
        # spectrum alone, which every slice shares; dk and dbias of the later slices are added to the first one's, in slice order
        dk_s = empty_like_rows(dk) if need_dk else None
        db_s = torch.empty_like(dbias) if need_dk else None
        for b0 in range(0, B, nb):
            b1, first = min(b0 + nb, B), b0 == 0
            check(lib().hyena_fftconv_bwd_ld(dout[b0:b1].data_ptr(), ptr(None if u is None else u[b0:b1]), None if saved is not None else ptr(k), bp,
                                             ptr(None if du is None else du[b0:b1]), ptr(dk if first else dk_s), ptr(dbias if first else db_s),
                                             b1 - b0, D, L, ldx, ldk, dtype_code(dout.dtype), tables.data_ptr(), ws.data_ptr(), ws.numel(),
                                             chunk, ptr(saved), saved.numel() if saved is not None else 0, stream))
            if need_dk and not first:
                dk += dk_s
                dbias += db_s
    return du, dk, dbias


# ---- fused mixer shell (include/hyena_mixer.h): short depthwise conv + gates + layout changes -----------------------
def mixer_pre_fwd(x, w, b, L):
    """x (B, Lx, 3D), w (3D, 3) fp32, b (3D,) fp32 -> vg (B, D, L) = short_conv(x)[v] * short_conv(x)[x1]."""
    _require_gpu(x, "x")
    B, Lx, D3 = x.shape
    D = D3 // 3
    vg = torch.empty((B, D, L), dtype=x.dtype, device=x.device)
    with _backend.guard(x.device):
        check(lib().hyena_mixer_pre_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), vg.data_ptr(), B, L, Lx, D,
                                        dtype_code(x.dtype), _backend.stream(x.device)))
    return vg


def mixer_post_fwd(y, x, w, b):
    """y (B, D, L), x (B, Lx, 3D) -> z (B, L, D) = y^T * short_conv(x)[x0]."""
    _require_gpu(x, "x")
    B, D, L = y.shape
    z = torch.empty((B, L, D), dtype=x.dtype, device=x.device)
    with _backend.guard(x.device):
        check(lib().hyena_mixer_post_fwd(y.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(), B, L,
                                         x.shape[1], D, dtype_code(x.dtype), _backend.stream(x.device)))
    return z


def mixer_partials(x, L):
    B, Lx, D3 = x.shape
    n = lib().hyena_mixer_partial_floats(B, L, D3 // 3)
    return torch.empty(n, dtype=torch.float32, device=x.device).view(B, -1, D3, 4)


def mixer_post_bwd(dz, y, x, w, b, dx, part):
    """-> dy (B, D, L); fills dx[..., 0:D] (positions < L) and part[..., 0:D, :]."""
    B, D, L = y.shape
    dy = torch.empty_like(y)
    with _backend.guard(x.device):
        check(lib().hyena_mixer_post_bwd(dz.data_ptr(), y.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(),
                                         dy.data_ptr(), dx.data_ptr(), part.data_ptr(), B, L, x.shape[1], D,
                                         dtype_code(x.dtype), _backend.stream(x.device)))
    return dy


def mixer_pre_bwd(dvg, x, w, b, dx, part):
    """fills dx[..., D:3D] (positions < L) and part[..., D:3D, :]."""
    B, D, L = dvg.shape
    with _backend.guard(x.device):
        check(lib().hyena_mixer_pre_bwd(dvg.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), dx.data_ptr(),
                                        part.data_ptr(), B, L, x.shape[1], D, dtype_code(x.dtype),
                                        _backend.stream(x.device)))


# ---- the shell in channel-major layout (include/hyena_mixer.h, hyena_cm_*) ------------------------------------------------
# xT / dxT / zT / dzT: any (cs, bs) layout (cm_strides); vg / y / dy / dvg: packed or pitched rows (ld_of).  What these functions allocate:
# empty_cm for the first kind, empty_rows for the second.
def cm_pre_fwd(xT, bin_, w, b, L):
    """xT (3D, B, Lx) [in_proj output without bias], bin_ (3D,) fp32 or None -> vg (B, D, L)."""
    _require_gpu(xT, "xT")
    D3, B, Lx = xT.shape
    D = D3 // 3
    xT = as_cm(xT)
    csx, bsx = cm_strides(xT)
    vg = empty_rows((B, D), L, xT.dtype, xT.device)
    with _backend.guard(xT.device):
        check(lib().hyena_cm_pre_fwd_ld(xT.data_ptr(), None if bin_ is None else bin_.data_ptr(), w.data_ptr(), b.data_ptr(), vg.data_ptr(),
                                        B, L, Lx, D, csx, bsx, ld_of(vg), dtype_code(xT.dtype), _backend.stream(xT.device)))
    return vg


def rows_as_cm_strides(t):
    """(cs, bs) that address a (B, D, L) tensor of pitched rows as rows (d, b): cs = its row pitch, bs = D times that (include/hyena_mixer.h)"""
    ld = ld_of(t)
    return ld, t.shape[1] * ld


def cm_post_fwd(y, xT, bin_, w, b, rows_out=False):
    """y (B, D, L), xT (3D, B, Lx) -> zT (D, B, L); rows_out: the same values as a (B, D, L) tensor of pitched rows (the next convolution's input
    when the operator's order is >= 3)."""
    B, D, L = y.shape
    xT, y = as_cm(xT), as_rows(y)
    csx, bsx = cm_strides(xT)
    if rows_out:
        zT = empty_like_rows(y, dtype=xT.dtype)
        csz, bsz = rows_as_cm_strides(zT)
    else:
        zT = empty_cm(D, B, L, xT.dtype, xT.device)
        csz, bsz = cm_strides(zT)
    with _backend.guard(xT.device):
        check(lib().hyena_cm_post_fwd_ld(y.data_ptr(), xT.data_ptr(), None if bin_ is None else bin_.data_ptr(), w.data_ptr(), b.data_ptr(),
                                         zT.data_ptr(), B, L, xT.shape[2], D, csx, bsx, csz, bsz, ld_of(y), dtype_code(xT.dtype),
                                         _backend.stream(xT.device)))
    return zT


def cm_partials(xT, L):
    D3, B, Lx = xT.shape
    n = lib().hyena_cm_partial_floats(B, L, D3 // 3)
    return torch.empty(n, dtype=torch.float32, device=xT.device).view(D3, -1, 8)


def cm_post_bwd(dzT, y, xT, bin_, w, b, dxT, part, dz_rows=False):
    """-> dy (B, D, L) with y's row pitch; fills dxT[0:D] (positions < L) and part[0:D].  dxT must have xT's layout.
    dz_rows: dzT is a (B, D, L) tensor of pitched rows (the gradient a convolution hands back for its input) instead of channel-major (D, B, L)."""
    B, D, L = y.shape
    xT, y = as_cm(xT), as_rows(y)
    csx, bsx = cm_strides(xT)
    if dz_rows:
        dzT = as_rows(dzT)
        assert tuple(dzT.shape) == (B, D, L)
        csz, bsz = rows_as_cm_strides(dzT)
    else:
        dzT = as_cm(dzT)
        csz, bsz = cm_strides(dzT)
    assert cm_strides(dxT) == (csx, bsx)
    dy = empty_like_rows(y)
    with _backend.guard(xT.device):
        check(lib().hyena_cm_post_bwd_ld(dzT.data_ptr(), y.data_ptr(), xT.data_ptr(), None if bin_ is None else bin_.data_ptr(), w.data_ptr(),
                                         b.data_ptr(), dy.data_ptr(), dxT.data_ptr(), part.data_ptr(), B, L, xT.shape[2], D,
                                         csx, bsx, csz, bsz, ld_of(y), dtype_code(xT.dtype), _backend.stream(xT.device)))
    return dy


def cm_pre_bwd(dvg, xT, bin_, w, b, dxT, part):
    """fills dxT[D:3D] (positions < L) and part[D:3D].  dxT must have xT's layout."""
    B, D, L = dvg.shape
    xT, dvg = as_cm(xT), as_rows(dvg)
    csx, bsx = cm_strides(xT)
    assert cm_strides(dxT) == (csx, bsx)
    with _backend.guard(xT.device):
        check(lib().hyena_cm_pre_bwd_ld(dvg.data_ptr(), xT.data_ptr(), None if bin_ is None else bin_.data_ptr(), w.data_ptr(), b.data_ptr(),
                                        dxT.data_ptr(), part.data_ptr(), B, L, xT.shape[2], D, csx, bsx, ld_of(dvg), dtype_code(xT.dtype),
                                        _backend.stream(xT.device)))


# ---- one decode position (include/hyena_decode.h): hist is the (Bcap, D, lda) history of the convolution's input, pos a one-int device tensor ----
DECODE_CHUNK = 8192          # history positions per decode_conv workgroup (DEC_CHUNK); the granularity of the fan-out's shared history


def decode_partials(B, D, Lcap, device):
    return torch.empty(lib().hyena_decode_partial_floats(int(B), int(D), int(Lcap)), dtype=torch.float32, device=device)


def _hist(hist):
    assert hist.dim() == 3 and hist.stride(2) == 1 and hist.stride(1) * hist.shape[1] == hist.stride(0)
    return hist.shape[0], hist.shape[1], hist.stride(1)


def decode_pre(x2, bin_, w, b, tail, hist, x0, pos, Lcap):
    """x2 (B, 3D) in_proj output of the new position without bias (rows contiguous) -> hist[:, :, t] = v * x1, x0 (B, D) fp32, tail shifted"""
    _require_gpu(x2, "x")
    B, D3 = x2.shape
    Bcap, D, lda = _hist(hist)
    assert D3 == 3 * D and x2.stride(1) == 1 and hist.dtype == x2.dtype
    with _backend.guard(x2.device):
        check(lib().hyena_decode_pre(x2.data_ptr(), x2.stride(0), None if bin_ is None else bin_.data_ptr(), w.data_ptr(), b.data_ptr(),
                                     tail.data_ptr(), hist.data_ptr(), x0.data_ptr(), pos.data_ptr(), B, Bcap, D, int(Lcap), lda,
                                     dtype_code(x2.dtype), _backend.stream(x2.device)))


def decode_conv(k, hist, part, pos, B, Lcap):
    """part[chunk][b][d] = the chunk's share of sum_{s <= t} k[d, t - s] hist[b, d, s]; k (D, ldk) fp32 rows contiguous"""
    _require_gpu(k, "k")
    _, D, lda = _hist(hist)
    assert k.dtype == torch.float32 and k.stride(1) == 1 and k.shape[0] == D
    with _backend.guard(k.device):
        check(lib().hyena_decode_conv(k.data_ptr(), k.stride(0), hist.data_ptr(), part.data_ptr(), pos.data_ptr(), int(B), D, int(Lcap), lda,
                                      dtype_code(hist.dtype), _backend.stream(k.device)))


def decode_post(part, hist, fb, x0, z, pos, B, Lcap):
    """z (B, D) = round(round(sum of the partials + fb hist[:, :, t]) * x0); advances pos"""
    _require_gpu(z, "z")
    _, D, lda = _hist(hist)
    assert z.dtype == hist.dtype and z.is_contiguous()
    with _backend.guard(z.device):
        check(lib().hyena_decode_post(part.data_ptr(), hist.data_ptr(), None if fb is None else fb.data_ptr(), x0.data_ptr(), z.data_ptr(),
                                      pos.data_ptr(), int(B), D, int(Lcap), lda, dtype_code(hist.dtype), _backend.stream(z.device)))


# ---- the same step with one position per row: pos a (>= B,) int32 device tensor, row b stands at pos[b]; rows outside [0, Lcap) are parked ----
def _pos_rows(pos, B):
    assert pos.dtype == torch.int32 and pos.dim() == 1 and pos.is_contiguous() and pos.shape[0] >= B


def decode_pre_rows(x2, bin_, w, b, tail, hist, x0, pos, Lcap):
    """decode_pre with t_b = pos[b]: hist[b, :, t_b] = v * x1 of row b, x0 (B, D) fp32, the tails of the rows that advance shifted"""
    _require_gpu(x2, "x")
    B, D3 = x2.shape
    Bcap, D, lda = _hist(hist)
    assert D3 == 3 * D and x2.stride(1) == 1 and hist.dtype == x2.dtype
    _pos_rows(pos, B)
    with _backend.guard(x2.device):
        check(lib().hyena_decode_pre_rows(x2.data_ptr(), x2.stride(0), None if bin_ is None else bin_.data_ptr(), w.data_ptr(), b.data_ptr(),
                                          tail.data_ptr(), hist.data_ptr(), x0.data_ptr(), pos.data_ptr(), B, Bcap, D, int(Lcap), lda,
                                          dtype_code(x2.dtype), _backend.stream(x2.device)))


def decode_conv_rows(k, hist, part, pos, B, Lcap):
    """part[chunk][b][d] = the chunk's share of sum_{s <= t_b} k[d, t_b - s] hist[b, d, s], written for the chunks that start at or below t_b"""
    _require_gpu(k, "k")
    _, D, lda = _hist(hist)
    assert k.dtype == torch.float32 and k.stride(1) == 1 and k.shape[0] == D
    _pos_rows(pos, B)
    with _backend.guard(k.device):
        check(lib().hyena_decode_conv_rows(k.data_ptr(), k.stride(0), hist.data_ptr(), part.data_ptr(), pos.data_ptr(), int(B), D, int(Lcap),
                                           lda, dtype_code(hist.dtype), _backend.stream(k.device)))


def decode_post_rows(part, hist, fb, x0, z, pos, B, Lcap):
    """z[b] = round(round(sum of row b's partials + fb hist[b, :, t_b]) * x0[b]); advances every pos[b] inside [0, Lcap)"""
    _require_gpu(z, "z")
    _, D, lda = _hist(hist)
    assert z.dtype == hist.dtype and z.is_contiguous()
    _pos_rows(pos, B)
    with _backend.guard(z.device):
        check(lib().hyena_decode_post_rows(part.data_ptr(), hist.data_ptr(), None if fb is None else fb.data_ptr(), x0.data_ptr(),
                                           z.data_ptr(), pos.data_ptr(), int(B), D, int(Lcap), lda, dtype_code(hist.dtype),
                                           _backend.stream(z.device)))


# ---- the same step for B = G fan rows (hyena_decode_*_fan): hist_s (G, D, lds) holds columns [0, S) of every group (None when S == 0),
# hist_r (Bcap, D, ldr) columns [S, Lcap) of every row, column t at index t - S; pos a one-int device tensor ----
def decode_pre_fan(x2, bin_, w, b, tail, hist_r, x0, pos, Lcap, S):
    """decode_pre with the new column written to hist_r[:, :, t - S]"""
    _require_gpu(x2, "x")
    B, D3 = x2.shape
    Bcap, D, ldr = _hist(hist_r)
    assert D3 == 3 * D and x2.stride(1) == 1 and hist_r.dtype == x2.dtype
    with _backend.guard(x2.device):
        check(lib().hyena_decode_pre_fan(x2.data_ptr(), x2.stride(0), None if bin_ is None else bin_.data_ptr(), w.data_ptr(), b.data_ptr(),
                                         tail.data_ptr(), hist_r.data_ptr(), x0.data_ptr(), pos.data_ptr(), B, Bcap, D, int(Lcap), int(S), ldr,
                                         dtype_code(x2.dtype), _backend.stream(x2.device)))


def decode_conv_fan(k, hist_s, hist_r, part, pos, B, fan, Lcap, S):
    """the partials of the chunks below S once per group, from hist_s, into part[chunk][g fan][d]; those from S on per row, from hist_r"""
    _require_gpu(k, "k")
    _, D, ldr = _hist(hist_r)
    lds = 0
    if hist_s is not None:
        G, Ds, lds = _hist(hist_s)
        assert Ds == D and hist_s.dtype == hist_r.dtype and G * int(fan) >= int(B)
    assert k.dtype == torch.float32 and k.stride(1) == 1 and k.shape[0] == D
    with _backend.guard(k.device):
        check(lib().hyena_decode_conv_fan(k.data_ptr(), k.stride(0), None if hist_s is None else hist_s.data_ptr(), hist_r.data_ptr(),
                                          part.data_ptr(), pos.data_ptr(), int(B), int(fan), D, int(Lcap), int(S), lds, ldr,
                                          dtype_code(hist_r.dtype), _backend.stream(k.device)))


def decode_post_fan(part, hist_r, fb, x0, z, pos, B, fan, Lcap, S):
    """decode_post with the partials of the chunks below S read from the group's slot and vg_t from hist_r[:, :, t - S]; advances pos"""
    _require_gpu(z, "z")
    _, D, ldr = _hist(hist_r)
    assert z.dtype == hist_r.dtype and z.is_contiguous()
    with _backend.guard(z.device):
        check(lib().hyena_decode_post_fan(part.data_ptr(), hist_r.data_ptr(), None if fb is None else fb.data_ptr(), x0.data_ptr(), z.data_ptr(),
                                          pos.data_ptr(), int(B), int(fan), D, int(Lcap), int(S), ldr, dtype_code(hist_r.dtype),
                                          _backend.stream(z.device)))


# ---- the block step (hyena_decode_*_block, *_block_fan): T positions per call.  x3 (B, T, 3D) the in_proj output without bias, x0 / z (B, T, D)
# contiguous, part from decode_block_partials; bit for bit what T single-position calls leave ----
DECODE_TMAX = 64             # HYENA_DECODE_TMAX: positions per block step


def decode_block_partials(B, D, Lcap, T, device):
    return torch.empty(lib().hyena_decode_block_partial_floats(int(B), int(D), int(Lcap), int(T)), dtype=torch.float32, device=device)


def _block_x(x3, hist):
    B, T, D3 = x3.shape
    assert x3.is_contiguous() and hist.dtype == x3.dtype and D3 == 3 * hist.shape[1]
    return B, T, D3


def _block_out(x0, z, B, T, D, hist):
    assert x0.dtype == torch.float32 and x0.shape == (B, T, D) and x0.is_contiguous()
    assert z is None or (z.dtype == hist.dtype and z.shape == (B, T, D) and z.is_contiguous())


def decode_pre_block(x3, bin_, w, b, tail, hist, x0, pos, Lcap):
    """hist[:, :, t0 ... t0 + T - 1] = v * x1 of the block's positions, x0 (B, T, D) fp32, tail = positions t0 + T - 2, t0 + T - 1"""
    _require_gpu(x3, "x")
    Bcap, D, lda = _hist(hist)
    B, T, ldx = _block_x(x3, hist)
    _block_out(x0, None, B, T, D, hist)
    with _backend.guard(x3.device):
        check(lib().hyena_decode_pre_block(x3.data_ptr(), ldx, None if bin_ is None else bin_.data_ptr(), w.data_ptr(), b.data_ptr(),
                                           tail.data_ptr(), hist.data_ptr(), x0.data_ptr(), pos.data_ptr(), B, Bcap, D, int(Lcap), lda, T,
                                           dtype_code(x3.dtype), _backend.stream(x3.device)))


def decode_conv_block(k, hist, part, pos, B, T, Lcap):
    """part[chunk][b][i][d] = the chunk's share of sum_{s <= t0 + i} k[d, t0 + i - s] hist[b, d, s]: the history is read once for the T outputs"""
    _require_gpu(k, "k")
    _, D, lda = _hist(hist)
    assert k.dtype == torch.float32 and k.stride(1) == 1 and k.shape[0] == D
    with _backend.guard(k.device):
        check(lib().hyena_decode_conv_block(k.data_ptr(), k.stride(0), hist.data_ptr(), part.data_ptr(), pos.data_ptr(), int(B), D, int(Lcap),
                                            lda, int(T), dtype_code(hist.dtype), _backend.stream(k.device)))


def decode_post_block(part, hist, fb, x0, z, pos, Lcap):
    """z (B, T, D) = round(round(sum of the partials + fb hist[:, :, t0 + i]) * x0); then pos = t0 + T"""
    _require_gpu(z, "z")
    _, D, lda = _hist(hist)
    B, T, _ = z.shape
    _block_out(x0, z, B, T, D, hist)
    with _backend.guard(z.device):
        check(lib().hyena_decode_post_block(part.data_ptr(), hist.data_ptr(), None if fb is None else fb.data_ptr(), x0.data_ptr(),
                                            z.data_ptr(), pos.data_ptr(), B, D, int(Lcap), lda, T, dtype_code(hist.dtype),
                                            _backend.stream(z.device)))


def decode_pre_block_fan(x3, bin_, w, b, tail, hist_r, x0, pos, Lcap, S):
    """decode_pre_block with the new columns written to hist_r[:, :, t0 - S ...]"""
    _require_gpu(x3, "x")
    Bcap, D, ldr = _hist(hist_r)
    B, T, ldx = _block_x(x3, hist_r)
    _block_out(x0, None, B, T, D, hist_r)
    with _backend.guard(x3.device):
        check(lib().hyena_decode_pre_block_fan(x3.data_ptr(), ldx, None if bin_ is None else bin_.data_ptr(), w.data_ptr(), b.data_ptr(),
                                               tail.data_ptr(), hist_r.data_ptr(), x0.data_ptr(), pos.data_ptr(), B, Bcap, D, int(Lcap), int(S),
                                               ldr, T, dtype_code(x3.dtype), _backend.stream(x3.device)))


def decode_conv_block_fan(k, hist_s, hist_r, part, pos, B, fan, T, Lcap, S):
    """decode_conv_block with the chunks below S computed once per group, from hist_s, into part[chunk][g fan]"""
    _require_gpu(k, "k")
    _, D, ldr = _hist(hist_r)
    lds = 0
    if hist_s is not None:
        G, Ds, lds = _hist(hist_s)
        assert Ds == D and hist_s.dtype == hist_r.dtype and G * int(fan) >= int(B)
    assert k.dtype == torch.float32 and k.stride(1) == 1 and k.shape[0] == D
    with _backend.guard(k.device):
        check(lib().hyena_decode_conv_block_fan(k.data_ptr(), k.stride(0), None if hist_s is None else hist_s.data_ptr(), hist_r.data_ptr(),
                                                part.data_ptr(), pos.data_ptr(), int(B), int(fan), D, int(Lcap), int(S), lds, ldr, int(T),
                                                dtype_code(hist_r.dtype), _backend.stream(k.device)))


def decode_post_block_fan(part, hist_r, fb, x0, z, pos, fan, Lcap, S):
    """decode_post_block with the partials of the chunks below S read from the group's slot; then pos = t0 + T"""
    _require_gpu(z, "z")
    _, D, ldr = _hist(hist_r)
    B, T, _ = z.shape
    _block_out(x0, z, B, T, D, hist_r)
    with _backend.guard(z.device):
        check(lib().hyena_decode_post_block_fan(part.data_ptr(), hist_r.data_ptr(), None if fb is None else fb.data_ptr(), x0.data_ptr(),
                                                z.data_ptr(), pos.data_ptr(), B, int(fan), D, int(Lcap), int(S), ldr, T,
                                                dtype_code(hist_r.dtype), _backend.stream(z.device)))


# ---- the lookahead carry (hyena_decode_carry, _conv_la, _post_la): carry (B, W, D) fp32 holds the share of outputs base ... base + W - 1 that
# comes from the history below base; pos and base one-int device tensors; the plain cache only ----
def decode_carry_partials(B, D, Lcap, W, device):
    return torch.empty(lib().hyena_decode_carry_partial_floats(int(B), int(D), int(Lcap), int(W)), dtype=torch.float32, device=device)


def _carry(carry, base, B, D):
    assert carry.dtype == torch.float32 and carry.dim() == 3 and carry.is_contiguous() and carry.shape[0] >= B and carry.shape[2] == D
    assert base.dtype == torch.int32 and base.numel() == 1
    return carry.shape[1]


def decode_carry(k, hist, part, carry, pos, base, B, Lcap):
    """carry[b, j, d] = sum_{s < t0} k[d, t0 + j - s] hist[b, d, s] for the W = carry.shape[1] outputs from t0 = pos on; then base = t0"""
    _require_gpu(k, "k")
    _, D, lda = _hist(hist)
    W = _carry(carry, base, B, D)
    assert k.dtype == torch.float32 and k.stride(1) == 1 and k.shape[0] == D
    with _backend.guard(k.device):
        check(lib().hyena_decode_carry(k.data_ptr(), k.stride(0), hist.data_ptr(), part.data_ptr(), carry.data_ptr(), pos.data_ptr(),
                                       base.data_ptr(), int(B), D, int(Lcap), lda, W, dtype_code(hist.dtype), _backend.stream(k.device)))


def decode_conv_la(k, hist, part, pos, base, B, W, Lcap):
    """decode_conv over s in [base, t] only: part (2, B, D), slot x for chunk base // 8192 + x"""
    _require_gpu(k, "k")
    _, D, lda = _hist(hist)
    assert k.dtype == torch.float32 and k.stride(1) == 1 and k.shape[0] == D and part.numel() >= 2 * int(B) * D
    with _backend.guard(k.device):
        check(lib().hyena_decode_conv_la(k.data_ptr(), k.stride(0), hist.data_ptr(), part.data_ptr(), pos.data_ptr(), base.data_ptr(), int(B), D,
                                         int(Lcap), lda, int(W), dtype_code(hist.dtype), _backend.stream(k.device)))


def decode_post_la(part, carry, hist, fb, x0, z, pos, base, B, Lcap):
    """z (B, D) = round(round(carry[:, t - base] + the live partials + fb hist[:, :, t]) * x0); advances pos"""
    _require_gpu(z, "z")
    _, D, lda = _hist(hist)
    W = _carry(carry, base, B, D)
    assert z.dtype == hist.dtype and z.is_contiguous()
    with _backend.guard(z.device):
        check(lib().hyena_decode_post_la(part.data_ptr(), carry.data_ptr(), hist.data_ptr(), None if fb is None else fb.data_ptr(),
                                         x0.data_ptr(), z.data_ptr(), pos.data_ptr(), base.data_ptr(), int(B), D, int(Lcap), lda, W,
                                         dtype_code(hist.dtype), _backend.stream(z.device)))


# ---- edited windows of a reference sequence (include/hyena_variant.h): M windows of T positions, window m starting at pos[m].  x3 (M, T, 3D) the
# in_proj output without bias, tail (3D, M, 2) fp32, pos (M,) int32, vg_ref (M, D, T) in x3's type, x0 (M, T, D) and delta / y_ref (M, D, T) fp32,
# z (M, T, D) in the I/O type; all contiguous ----
VARIANT_TMAX = 1024          # HYENA_VARIANT_TMAX: positions per window


def variant_pre(x3, bin_, w, b, tail, pos, vg_ref, x0, delta):
    """x0 = the gate, delta = float(round_io(v * x1)) - float(vg_ref) of every window position; -> VARIANT_TMAX"""
    _require_gpu(x3, "x")
    M, T, D3 = x3.shape
    D = D3 // 3
    assert x3.is_contiguous() and D3 == 3 * D and vg_ref.dtype == x3.dtype and vg_ref.shape == (M, D, T) and vg_ref.is_contiguous()
    assert tail.dtype == torch.float32 and tail.shape == (D3, M, 2) and tail.is_contiguous()
    assert pos.dtype == torch.int32 and pos.shape == (M,) and pos.is_contiguous()
    assert x0.dtype == torch.float32 and x0.shape == (M, T, D) and x0.is_contiguous()
    assert delta.dtype == torch.float32 and delta.shape == (M, D, T) and delta.is_contiguous()
    with _backend.guard(x3.device):
        check(lib().hyena_variant_pre(x3.data_ptr(), D3, None if bin_ is None else bin_.data_ptr(), w.data_ptr(), b.data_ptr(), tail.data_ptr(),
                                      pos.data_ptr(), vg_ref.data_ptr(), x0.data_ptr(), delta.data_ptr(), M, D, T, dtype_code(x3.dtype),
                                      _backend.stream(x3.device)))
    return VARIANT_TMAX


def variant_conv(y_ref, delta, k, fb, x0, z):
    """z (M, T, D) = round(round(y_ref + the causal product of k[:, :T] with delta + fb delta) * x0); k (D, >= T) fp32 rows contiguous; -> VARIANT_TMAX"""
    _require_gpu(z, "z")
    M, T, D = z.shape
    assert z.is_contiguous() and z.dtype in _DTYPES
    assert k.dtype == torch.float32 and k.dim() == 2 and k.stride(1) == 1 and k.shape[0] == D and k.shape[1] >= T
    for t in (y_ref, delta):
        assert t.dtype == torch.float32 and t.shape == (M, D, T) and t.is_contiguous()
    assert x0.dtype == torch.float32 and x0.shape == (M, T, D) and x0.is_contiguous()
    with _backend.guard(z.device):
        check(lib().hyena_variant_conv(y_ref.data_ptr(), delta.data_ptr(), k.data_ptr(), k.stride(0) if D > 1 else max(k.shape[1], T),
                                       None if fb is None else fb.data_ptr(), x0.data_ptr(), z.data_ptr(), M, D, T, dtype_code(z.dtype),
                                       _backend.stream(z.device)))
    return VARIANT_TMAX



# ---- token sampling, the last node of the per-token step (hyena_decode_sample): one wavefront per logit row ------------------------------------
SAMPLE_MAX_V = 64
AUTOMATON_MAX_STATES = 4096  # HYENA_DECODE_AUTOMATON_MAX_STATES: states of a token automaton
AUTOMATON_MAX_TABLE = 1 << 22  # HYENA_DECODE_AUTOMATON_MAX_TABLE: entries Nt S of its step table M


def _automaton_tables(automaton, B, V, dev):
    """(M (Nt, S) int64, delta (S, V) int32, dstate (B,) int32), all contiguous on ``dev`` -> the six arguments of the C entry points"""
    M, delta, dstate = automaton
    assert M.dtype == torch.int64 and M.dim() == 2 and M.is_contiguous() and M.shape[0] >= 1
    assert delta.dtype == torch.int32 and delta.dim() == 2 and delta.is_contiguous() and delta.shape[0] == M.shape[1]
    assert dstate.dtype == torch.int32 and dstate.shape == (B,) and dstate.is_contiguous()
    assert M.device == delta.device == dstate.device == dev
    return M.data_ptr(), M.shape[0], M.shape[1], delta.data_ptr(), delta.shape[1], dstate.data_ptr()


def decode_sample(logits, seed, col, done, seq, nxt, temperature=1.0, top_k=1, top_p=1.0, eos=-1, pad=0, vocab=None, scores=None, u_out=None,
                  allow=None, start=None, logprobs=None, automaton=None):
    """logits (B, V <= 64) fp32 / bf16 / fp16, rows contiguous -> row b's token at seq[b, col[b]] and nxt[b]; col advanced, done set on `eos`
    (< 0: none); a parked row (col outside seq's columns) is left alone, a done row only gets nxt[b] = pad.  ``seed``: device int64 (1,);
    ``col`` / ``done``: device int32 (B,); ``seq`` (B, ncols) and ``nxt`` (B,) or (B, 1): int64; ``vocab``: the live columns (default V);
    ``scores`` (B, ncols, V) fp32 or None receives logits / T at [b, col[b]]; ``u_out`` (B,) fp32 or None the uniform each row drew.

    ``allow`` / ``start`` / ``logprobs`` all None: hyena_decode_sample.  Otherwise hyena_decode_sample_constrained: ``start`` int32 (B,) the
    column of every row's first new token; ``allow`` int64 bit masks (N,) -- one row for the batch -- or (B, N), bit v of allow[b, i]: token
    v may be row b's i-th new token (an empty mask, or i outside [0, N): unconstrained); ``logprobs`` (B, N') fp32 receives at
    [b, col[b] - start[b]] the emitted token's log-probability under the softmax of the live logits at temperature 1.

    ``automaton`` = (M, delta, dstate): hyena_decode_sample_automaton -- row b's mask is M[n, dstate[b]] (M (Nt, S) int64; Nt == 1: M[0] for
    every n), and dstate[b] (int32 (B,)) moves on to delta[dstate[b], token] (delta (S, V) int32, -1: forbidden).  Needs ``start``; not
    together with ``allow`` (positional masks are folded into M)."""
    _require_gpu(logits, "logits")
    assert logits.dim() == 2 and logits.stride(1) == 1
    B, V = logits.shape
    assert seed.dtype == torch.int64 and seed.numel() == 1
    for t in (col, done):
        assert t.dtype == torch.int32 and t.shape == (B,) and t.is_contiguous()
    assert seq.dtype == torch.int64 and seq.dim() == 2 and seq.shape[0] == B and seq.stride(1) == 1
    ncols = seq.shape[1]
    assert nxt.dtype == torch.int64 and nxt.numel() == B and nxt.shape[0] == B
    assert scores is None or (scores.dtype == torch.float32 and scores.shape == (B, ncols, V) and scores.is_contiguous())
    assert u_out is None or (u_out.dtype == torch.float32 and u_out.shape == (B,) and u_out.is_contiguous())
    for t in (seed, col, done, seq, nxt, scores, u_out):
        assert t is None or t.device == logits.device
    if automaton is not None:
        assert allow is None and start is not None and start.dtype == torch.int32 and start.shape == (B,) and start.is_contiguous()
        assert logprobs is None or (logprobs.dtype == torch.float32 and logprobs.dim() == 2 and logprobs.shape[0] == B
                                    and logprobs.shape[1] >= 1 and logprobs.is_contiguous())
        assert start.device == logits.device and (logprobs is None or logprobs.device == logits.device)
        with _backend.guard(logits.device):
            check(lib().hyena_decode_sample_automaton(
                logits.data_ptr(), logits.stride(0) if B > 1 else V, dtype_code(logits.dtype), B, V, V if vocab is None else int(vocab),
                float(temperature), int(top_k), float(top_p), seed.data_ptr(), int(eos), int(pad), col.data_ptr(), done.data_ptr(),
                seq.data_ptr(), seq.stride(0) if B > 1 else ncols, ncols, nxt.data_ptr(), nxt.stride(0) if B > 1 else 1,
                None if scores is None else scores.data_ptr(), None if u_out is None else u_out.data_ptr(),
                *_automaton_tables(automaton, B, V, logits.device), start.data_ptr(), None if logprobs is None else logprobs.data_ptr(),
                0 if logprobs is None else logprobs.shape[1], _backend.stream(logits.device)))
        return
    if allow is not None or start is not None or logprobs is not None:
        assert start is not None and start.dtype == torch.int32 and start.shape == (B,) and start.is_contiguous()
        assert allow is None or (allow.dtype == torch.int64 and allow.dim() in (1, 2) and allow.shape[-1] >= 1 and allow.is_contiguous()
                                 and (allow.dim() == 1 or allow.shape[0] == B))
        assert logprobs is None or (logprobs.dtype == torch.float32 and logprobs.dim() == 2 and logprobs.shape[0] == B
                                    and logprobs.shape[1] >= 1 and logprobs.is_contiguous())
        for t in (allow, start, logprobs):
            assert t is None or t.device == logits.device
        with _backend.guard(logits.device):
            check(lib().hyena_decode_sample_constrained(
                logits.data_ptr(), logits.stride(0) if B > 1 else V, dtype_code(logits.dtype), B, V, V if vocab is None else int(vocab),
                float(temperature), int(top_k), float(top_p), seed.data_ptr(), int(eos), int(pad), col.data_ptr(), done.data_ptr(),
                seq.data_ptr(), seq.stride(0) if B > 1 else ncols, ncols, nxt.data_ptr(), nxt.stride(0) if B > 1 else 1,
                None if scores is None else scores.data_ptr(), None if u_out is None else u_out.data_ptr(),
                None if allow is None else allow.data_ptr(), 0 if allow is None or allow.dim() == 1 else allow.shape[1],
                0 if allow is None else allow.shape[-1], start.data_ptr(), None if logprobs is None else logprobs.data_ptr(),
                0 if logprobs is None else logprobs.shape[1], _backend.stream(logits.device)))
        return
    with _backend.guard(logits.device):
        check(lib().hyena_decode_sample(logits.data_ptr(), logits.stride(0) if B > 1 else V, dtype_code(logits.dtype), B, V,
                                        V if vocab is None else int(vocab), float(temperature), int(top_k), float(top_p), seed.data_ptr(),
                                        int(eos), int(pad), col.data_ptr(), done.data_ptr(), seq.data_ptr(), seq.stride(0) if B > 1 else ncols,
                                        ncols, nxt.data_ptr(), nxt.stride(0) if B > 1 else 1, None if scores is None else scores.data_ptr(),
                                        None if u_out is None else u_out.data_ptr(), _backend.stream(logits.device)))


# ---- beam search over the fan-out layout (hyena_decode_beam, hyena_decode_reorder_fan, hyena_decode_beam_backtrack) ----------------------------
DECODE_BEAM_MAX = 16         # HYENA_DECODE_BEAM_MAX: beams per prompt (the rows of a fan group)


def _beam_rows(B, fan, *tensors):
    assert 1 <= int(fan) <= DECODE_BEAM_MAX and B % int(fan) == 0
    for t in tensors:
        assert t.dtype == torch.int32 and t.shape == (B,) and t.is_contiguous()


def decode_beam(logits, score, col, done, start, parent, nxt, fan, ncols, eos=-1, pad=0, vocab=None, allow=None, tok_hist=None, parent_hist=None,
                lp_hist=None, automaton=None):
    """The beam step: logits (B = G fan, V <= 64) fp32 / bf16 / fp16, rows contiguous; the ``fan`` rows of a group are the beams of one
    prompt, best first.  ``score`` fp32 (B,) cumulative log-probabilities (0 / -inf ... before the first step); ``col`` / ``done`` /
    ``start`` / ``parent``: device int32 (B,); ``nxt`` (B,) or (B, 1) int64.  Per group the ``fan`` best of {live row, allowed token} and
    {finished row, pad} by score (then NaN scores; ties by row, then token) go to its rows in rank order: ``parent`` (absolute row),
    ``score``, ``done``, ``nxt``, ``col`` + 1 and the records ``tok_hist`` / ``parent_hist`` (int32) / ``lp_hist`` (fp32), all (B, N'), at
    [b, col[b] - start[b]].  A group whose column lies outside [0, ncols) is left alone.  ``allow``: as for ``decode_sample``.
    ``automaton`` = (M, delta, dstate), not together with ``allow``: hyena_decode_beam_automaton -- row b's allowed set is M[n, dstate[b]],
    and rank r receives the state delta[dstate[parent], token] (its parent's as it is for pad and eos)."""
    _require_gpu(logits, "logits")
    assert logits.dim() == 2 and logits.stride(1) == 1
    B, V = logits.shape
    _beam_rows(B, fan, col, done, start, parent)
    assert score.dtype == torch.float32 and score.shape == (B,) and score.is_contiguous()
    assert nxt.dtype == torch.int64 and nxt.numel() == B and nxt.shape[0] == B
    assert allow is None or (allow.dtype == torch.int64 and allow.dim() in (1, 2) and allow.shape[-1] >= 1 and allow.is_contiguous()
                             and (allow.dim() == 1 or allow.shape[0] == B))
    recs = [t for t in (tok_hist, parent_hist, lp_hist) if t is not None]
    for t in recs:
        assert t.dim() == 2 and t.shape == (B, recs[0].shape[1]) and t.shape[1] >= 1 and t.is_contiguous()
        assert t.dtype == (torch.float32 if t is lp_hist else torch.int32)
    for t in [score, col, done, start, parent, nxt, allow] + recs:
        assert t is None or t.device == logits.device
    nrec = recs[0].shape[1] if recs else 0
    if automaton is not None:
        assert allow is None
        with _backend.guard(logits.device):
            check(lib().hyena_decode_beam_automaton(
                logits.data_ptr(), logits.stride(0) if B > 1 else V, dtype_code(logits.dtype), B, int(fan), V, V if vocab is None else int(vocab),
                int(eos), int(pad), col.data_ptr(), done.data_ptr(), score.data_ptr(), start.data_ptr(), parent.data_ptr(), nxt.data_ptr(),
                nxt.stride(0) if B > 1 else 1, int(ncols), *_automaton_tables(automaton, B, V, logits.device),
                None if tok_hist is None else tok_hist.data_ptr(), None if parent_hist is None else parent_hist.data_ptr(),
                None if lp_hist is None else lp_hist.data_ptr(), nrec, nrec, _backend.stream(logits.device)))
        return
    with _backend.guard(logits.device):
        check(lib().hyena_decode_beam(
            logits.data_ptr(), logits.stride(0) if B > 1 else V, dtype_code(logits.dtype), B, int(fan), V, V if vocab is None else int(vocab),
            int(eos), int(pad), col.data_ptr(), done.data_ptr(), score.data_ptr(), start.data_ptr(), parent.data_ptr(), nxt.data_ptr(),
            nxt.stride(0) if B > 1 else 1, int(ncols), None if allow is None else allow.data_ptr(),
            0 if allow is None or allow.dim() == 1 else allow.shape[1], 0 if allow is None else allow.shape[-1],
            None if tok_hist is None else tok_hist.data_ptr(), None if parent_hist is None else parent_hist.data_ptr(),
            None if lp_hist is None else lp_hist.data_ptr(), nrec, nrec, _backend.stream(logits.device)))


def decode_reorder_fan(hist_r, tail, parent, pos, B, fan, Lcap, S, c0):
    """in place: hist_r[b, :, s - S] = old hist_r[parent[b], :, s - S] for c0 <= s < *pos, tail[:, b] = old tail[:, parent[b]] for every
    row b < B (a parent outside b's group: b itself); nothing at all when *pos lies outside [S, Lcap]"""
    _require_gpu(hist_r, "history")
    Bcap, D, ldr = _hist(hist_r)
    _beam_rows(int(B), fan, parent)
    assert tail.dtype == torch.float32 and tail.shape == (3 * D, Bcap, 2) and tail.is_contiguous()
    assert pos.dtype == torch.int32 and pos.numel() >= 1 and parent.device == hist_r.device == tail.device == pos.device
    with _backend.guard(hist_r.device):
        check(lib().hyena_decode_reorder_fan(hist_r.data_ptr(), tail.data_ptr(), parent.data_ptr(), pos.data_ptr(), int(B), Bcap, int(fan), D,
                                             int(Lcap), int(S), int(c0), ldr, dtype_code(hist_r.dtype), _backend.stream(hist_r.device)))


def decode_beam_backtrack(tok_hist, parent_hist, lp_hist, fan, n_done, n_ret, seq, P, logprobs=None):
    """seq[g n_ret + r, P + i] (and logprobs[g n_ret + r, i]) for i < n_done: the tokens (log-probs) of the beam that ends in row g fan + r,
    read off the records backwards through ``parent_hist``"""
    _require_gpu(tok_hist, "tok_hist")
    B = tok_hist.shape[0]
    assert 1 <= int(fan) <= DECODE_BEAM_MAX and B % int(fan) == 0 and 1 <= int(n_ret) <= int(fan)
    for t in (tok_hist, parent_hist):
        assert t.dtype == torch.int32 and t.dim() == 2 and t.shape == tok_hist.shape and t.is_contiguous()
    rows = B // int(fan) * int(n_ret)
    assert seq.dtype == torch.int64 and seq.dim() == 2 and seq.shape[0] == rows and seq.stride(1) == 1 and seq.device == tok_hist.device
    assert 0 <= int(n_done) <= tok_hist.shape[1] and int(P) >= 0 and seq.shape[1] >= int(P) + int(n_done)
    if logprobs is not None:
        assert lp_hist is not None and lp_hist.dtype == torch.float32 and lp_hist.shape == tok_hist.shape and lp_hist.is_contiguous()
        assert logprobs.dtype == torch.float32 and logprobs.dim() == 2 and logprobs.shape[0] == rows and logprobs.stride(1) == 1
        assert logprobs.shape[1] >= max(int(n_done), 1) and logprobs.device == tok_hist.device
    with _backend.guard(tok_hist.device):
        check(lib().hyena_decode_beam_backtrack(
            tok_hist.data_ptr(), parent_hist.data_ptr(), None if lp_hist is None else lp_hist.data_ptr(), tok_hist.stride(0), B, int(fan),
            int(n_done), int(n_ret), seq.data_ptr(), seq.stride(0) if rows > 1 else seq.shape[1], int(P),
            None if logprobs is None else logprobs.data_ptr(), 0 if logprobs is None else (logprobs.stride(0) if rows > 1 else logprobs.shape[1]),
            _backend.stream(tok_hist.device)))


# ---- input projection on the matrix cores with the front of the shell in its epilogue (include/hyena_proj.h) --------------------
def proj_supported(B, Lx, D, dtype):
    code = _DTYPES.get(dtype)
    return code is not None and bool(lib().hyena_proj_supported(int(B), int(Lx), int(D), code)) and row_pitch(B * Lx) < 2 ** 31


def inproj_pre_fwd(u, W, bin_, w, b, L):
    """u (B, Lx, D) 16-bit, W (3D, D) same type, bin_ (3D,) fp32 or None, w (3D, 3) fp32, b (3D,) fp32
    -> xT (3D, B, Lx) = W u^T (no bias; empty_cm layout), vg (B, D, L) = short_conv(xT + bin_)[v] * short_conv(xT + bin_)[x1] (pitched rows)."""
    _require_gpu(u, "u")
    B, Lx, D = u.shape
    assert W.shape == (3 * D, D) and W.dtype == u.dtype and u.is_contiguous() and W.is_contiguous()
    xT = empty_cm(3 * D, B, Lx, u.dtype, u.device)
    csx, bsx = cm_strides(xT)
    vg = empty_rows((B, D), L, u.dtype, u.device)
    with _backend.guard(u.device):
        check(lib().hyena_inproj_pre_fwd_ld(u.data_ptr(), W.data_ptr(), None if bin_ is None else bin_.data_ptr(), w.data_ptr(), b.data_ptr(),
                                            xT.data_ptr(), vg.data_ptr(), B, Lx, int(L), D, csx, bsx, ld_of(vg), dtype_code(u.dtype),
                                            _backend.stream(u.device)))
    return xT, vg


def proj_kernel_generation(family, generation=0):
    """include/hyena_proj.h, hyena_proj_kernel_generation: family 0 = out_proj forward, 1 = in_proj forward; generation 0 queries, 1 / 2 selects
    (process-wide)."""
    return int(lib().hyena_proj_kernel_generation(int(family), int(generation)))


def outproj_supported(B, L, Lx, D, dtype):
    code = _DTYPES.get(dtype)
    return code is not None and code != 0 and Lx >= L and bool(lib().hyena_outproj_supported(int(B), int(L), int(D), code))


def outproj_gate_fwd(y, xT, bin_, w, b, W, bias, want_z):
    """y (B, D, L) conv output, xT (3D, B, Lx), bin_ / w / b as cm_post_fwd, W (D, D) out_proj weight (element type of y), bias (D,) fp32
    [values already rounded to the element type] or None -> out (B, L, D) = (y * x0)^T W^T + bias (packed), zT (D, B, L) = y * x0 (empty_cm
    layout) if want_z else None (bit-identical to cm_post_fwd).  One launch: the gate rides on the operand load of the matrix-core product."""
    out, _, _, _, zT = _outproj(y, xT, bin_, w, b, W, bias, want_z, None)
    return out, zT


def outproj_gate_addnorm_fwd(y, xT, bin_, w, b, W, bias, want_z, residual, ln_w, ln_b, eps):
    """outproj_gate_fwd with the block's residual add + LayerNorm in the kernel's epilogue (include/hyena_proj.h,
    hyena_outproj_gate_addnorm_fwd_ld): residual (B L, D) fp32 or None, ln_w / ln_b (D,) fp32
    -> normed (B, L, D) of y's type, residual' (B L, D) fp32, mean, rstd (B L,), zT or None.  The out_proj output itself is never written."""
    return _outproj(y, xT, bin_, w, b, W, bias, want_z, (residual, ln_w, ln_b, eps))


def _outproj(y, xT, bin_, w, b, W, bias, want_z, norm):
    _require_gpu(y, "y")
    B, D, L = y.shape
    y, xT = as_rows(y), as_cm(xT)
    assert W.shape == (D, D) and W.dtype == y.dtype and xT.dtype == y.dtype and W.is_contiguous()
    dev = y.device
    csx, bsx = cm_strides(xT)
    out = torch.empty((B, L, D), dtype=y.dtype, device=dev)
    zT = empty_cm(D, B, L, y.dtype, dev) if want_z else None
    csz, bsz = cm_strides(zT) if want_z else (0, 0)
    res_out = mean = rstd = residual = ln_w = ln_b = None
    eps = 0.0
    if norm is not None:
        residual, ln_w, ln_b, eps = norm
        assert residual is None or (residual.dtype == torch.float32 and residual.is_contiguous() and residual.numel() == B * L * D)
        res_out = torch.empty((B * L, D), dtype=torch.float32, device=dev)
        mean = torch.empty(B * L, dtype=torch.float32, device=dev)
        rstd = torch.empty(B * L, dtype=torch.float32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    with _backend.guard(dev):
        check(lib().hyena_outproj_gate_addnorm_fwd_ld(y.data_ptr(), xT.data_ptr(), ptr(bin_), w.data_ptr(), b.data_ptr(), W.data_ptr(), ptr(bias),
                                                      ptr(residual), ptr(ln_w), ptr(ln_b), float(eps), out.data_ptr(), ptr(res_out), ptr(mean),
                                                      ptr(rstd), ptr(zT), B, L, xT.shape[2], D, csx, bsx, csz, bsz, ld_of(y),
                                                      dtype_code(y.dtype), _backend.stream(dev)))
    return out, res_out, mean, rstd, zT


def outproj_dgrad_supported(B, L, D, dtype):
    code = _DTYPES.get(dtype)
    return code is not None and code != 0 and bool(lib().hyena_outproj_dgrad_supported(int(B), int(L), int(D), code))


def outproj_dgrad_gate_bwd(dy2, WoT, y, xT, bin_, w, b, dxT):
    """out_proj's input gradient with cm_post_bwd's work in the kernel's epilogue (include/hyena_proj.h, hyena_outproj_dgrad_gate_bwd_ld):
    dy2 (B L, D) 16-bit, WoT (D, D) = out_proj.weight^T contiguous, y (B, D, L), xT (3D, B, Lx); fills dxT[0:D] (positions < L)
    -> dyc (B, D, L) with y's row pitch, part0 (D, runs, 8) whose [:, :, :5].sum(1) are (dw0, dw1, dw2, db_sc, db_in) of channels [0, D)."""
    _require_gpu(y, "y")
    B, D, L = y.shape
    y, xT = as_rows(y), as_cm(xT)
    assert dy2.shape == (B * L, D) and dy2.is_contiguous() and dy2.dtype == y.dtype and WoT.shape == (D, D) and WoT.is_contiguous()
    csx, bsx = cm_strides(xT)
    assert cm_strides(dxT) == (csx, bsx)
    dyc = empty_like_rows(y)
    part = torch.empty(lib().hyena_outproj_dgrad_partial_floats(B, L, D), dtype=torch.float32, device=y.device).view(D, -1, 8)
    with _backend.guard(y.device):
        check(lib().hyena_outproj_dgrad_gate_bwd_ld(dy2.data_ptr(), WoT.data_ptr(), y.data_ptr(), xT.data_ptr(),
                                                    None if bin_ is None else bin_.data_ptr(), w.data_ptr(), b.data_ptr(), dyc.data_ptr(),
                                                    dxT.data_ptr(), part.data_ptr(), B, L, xT.shape[2], D, csx, bsx, ld_of(y),
                                                    dtype_code(y.dtype), _backend.stream(y.device)))
    return dyc, part


def colsum(x2):
    """x2 (P, N) 16-bit contiguous -> (N,) fp32 = x2.sum(0) (the bias gradient of a linear layer) in one pass at the memory rate;
    falls back to torch's reduction for shapes the kernel does not serve (and for host tensors outside the test double)."""
    P, N = x2.shape
    from . import _gradsum
    got = _gradsum.take(x2)              # the tensor's producer (add_norm_bwd) may have summed its columns already
    if got is not None:
        return got
    code = _DTYPES.get(x2.dtype)
    if code is None or not (x2.is_cuda or _backend.name != "hip") or not x2.is_contiguous() or not lib().hyena_colsum_supported(P, N, code):
        return x2.sum(0, dtype=torch.float32)
    out = torch.empty(N, dtype=torch.float32, device=x2.device)
    part = torch.empty(lib().hyena_colsum_partial_floats(P, N), dtype=torch.float32, device=x2.device)
    with _backend.guard(x2.device):
        check(lib().hyena_colsum(x2.data_ptr(), part.data_ptr(), out.data_ptr(), P, N, code, _backend.stream(x2.device)))
    return out


def mlp_supported(P, K, N, dtype):
    code = _DTYPES.get(dtype)
    return code is not None and bool(lib().hyena_mlp_supported(int(P), int(K), int(N), code))


def mlp_fc1_gelu_fwd(x2, W1, b1):
    """x2 (P, K) 16-bit, W1 (N, K) same type, b1 (N,) fp32 (values already rounded to the element type) or None
    -> a = x2 W1^T + b1, h = gelu_tanh(a), both (P, N)."""
    _require_gpu(x2, "x")
    P, K = x2.shape
    N = W1.shape[0]
    a = torch.empty((P, N), dtype=x2.dtype, device=x2.device)
    h = torch.empty((P, N), dtype=x2.dtype, device=x2.device)
    with _backend.guard(x2.device):
        check(lib().hyena_mlp_fc1_gelu_fwd(x2.data_ptr(), W1.data_ptr(), None if b1 is None else b1.data_ptr(), a.data_ptr(), h.data_ptr(),
                                           P, K, N, dtype_code(x2.dtype), _backend.stream(x2.device)))
    return a, h


def mlp_dh_dgelu_bwd(dy2, W2T, a):
    """dy2 (P, K), W2T (N, K) = fc2.weight^T contiguous, a (P, N) -> da (P, N) = (dy2 W2) * gelu_tanh'(a), db1 (N,) fp32 = da.sum(0)."""
    _require_gpu(dy2, "dy")
    P, K = dy2.shape
    N = W2T.shape[0]
    da = torch.empty((P, N), dtype=dy2.dtype, device=dy2.device)
    part = torch.empty(lib().hyena_mlp_partial_floats(P, N), dtype=torch.float32, device=dy2.device)
    with _backend.guard(dy2.device):
        check(lib().hyena_mlp_dh_dgelu_bwd(dy2.data_ptr(), W2T.data_ptr(), a.data_ptr(), da.data_ptr(), part.data_ptr(), P, K, N,
                                           dtype_code(dy2.dtype), _backend.stream(dy2.device)))
    return da, part.view(-1, N).sum(0)                          # fixed-order two-stage sum: deterministic


# ---- fused implicit filter (include/hyena_filter.h) ---------------------------------------------------------------------
def filter_supported(L, E, order, D):
    return bool(lib().hyena_filter_supported(int(L), int(E), int(order), int(D)))


def _filter_params(z, t, w0, b0, w1, b1, w2, b2, w3, freq, deltas, shift, modulate):
    L, E = z.shape
    p = FilterParams()
    for name, ten in (("z", z), ("t", t), ("w0", w0), ("b0", b0), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("w3", w3),
                      ("freq", freq), ("deltas", deltas)):
        if ten is not None:
            _require_gpu(ten, name)
            assert ten.dtype == torch.float32 and ten.is_contiguous(), name
        setattr(p, name, None if ten is None else ten.data_ptr())
    p.shift, p.modulate, p.z_stride, p.L, p.E, p.D = float(shift), int(bool(modulate)), z.stride(0), L, E, w3.shape[0]
    return p


def filter_fwd(z, t, w0, b0, w1, b1, w2, b2, w3, freq, deltas, shift, modulate, save, compute_dtype=None):
    """z (L, E), t (L,), weights as in include/hyena_filter.h -> k (D, L) fp32, pitched rows [, saved pre-activations].  ``compute_dtype``
    bfloat16 / float16: the graph the reference computes under torch.autocast of that type (hyena_filter16_fwd; the pre-activations are
    kept as (3, 32, P) 32-bit words holding 16-bit pairs, P = the library's row pitch for L); None: the fp32 graph ((3, 64, P) fp32)."""
    p = _filter_params(z, t, w0, b0, w1, b1, w2, b2, w3, freq, deltas, shift, modulate)
    k = empty_rows((p.D,), p.L, torch.float32, z.device)
    P = int(lib().hyena_filter_row_pitch(p.L))
    if compute_dtype is None:
        saved = torch.empty((3, 64, P), dtype=torch.float32, device=z.device) if save else None
    else:
        saved = torch.empty((3, 32, P), dtype=torch.int32, device=z.device) if save else None
    with _backend.guard(z.device):
        sp = None if saved is None else saved.data_ptr()
        if compute_dtype is None:
            check(lib().hyena_filter_fwd_ld(ctypes.byref(p), k.data_ptr(), ld_of(k), sp, _backend.stream(z.device)))
        else:
            check(lib().hyena_filter16_fwd_ld(ctypes.byref(p), dtype_code(compute_dtype), k.data_ptr(), ld_of(k), sp,
                                              _backend.stream(z.device)))
    return (k, saved) if save else k


def filter_bwd(dk, saved, z, t, w0, b0, w1, b1, w2, b2, w3, freq, deltas, shift, modulate, need_dz, compute_dtype=None):
    """-> (dw0, db0, dw1, db1, dw2, db2, dw3, dfreq, dz or None); dz is (L, E).  dk (D, L) fp32, packed or pitched rows.  ``compute_dtype`` as
    in filter_fwd (``saved`` must come from the forward of the same type)."""
    p = _filter_params(z, t, w0, b0, w1, b1, w2, b2, w3, freq, deltas, shift, modulate)
    _require_gpu(dk, "dk")
    assert dk.dtype == torch.float32 and dk.shape == (p.D, p.L)
    dk = as_rows(dk)
    outs = [torch.empty_like(x) for x in (w0, b0, w1, b1, w2, b2, w3, freq)]
    dzt = torch.empty((p.E, p.L), dtype=torch.float32, device=z.device) if need_dz else None
    g = FilterGrads()
    for name, ten in zip(("dw0", "db0", "dw1", "db1", "dw2", "db2", "dw3", "dfreq"), outs):
        setattr(g, name, ten.data_ptr())
    g.dz = None if dzt is None else dzt.data_ptr()
    nbytes = lib().hyena_filter_workspace_bytes(p.L, p.D)
    with _backend.guard(z.device):
        ws, stream = workspace_for(z.device, nbytes)
        if compute_dtype is None:
            assert saved.dtype == torch.float32
            check(lib().hyena_filter_bwd_ld(ctypes.byref(p), dk.data_ptr(), ld_of(dk), saved.data_ptr(), ctypes.byref(g), ws.data_ptr(),
                                            ws.numel(), stream))
        else:
            assert saved.dtype == torch.int32
            check(lib().hyena_filter16_bwd_ld(ctypes.byref(p), dtype_code(compute_dtype), dk.data_ptr(), ld_of(dk), saved.data_ptr(),
                                              ctypes.byref(g), ws.data_ptr(), ws.numel(), stream))
    return tuple(outs) + (None if dzt is None else dzt.t().contiguous(),)


# ---- fused residual add + LayerNorm of a block (include/hyena_block.h) ------------------------------------------------
def add_norm_supported(D, x_dtype, out_dtype):
    try:
        return bool(lib().hyena_add_norm_supported(int(D), dtype_code(x_dtype), dtype_code(out_dtype)))
    except TypeError:
        return False


def add_norm_fwd(x0, residual, weight, bias, eps, out_dtype, dropout_p=0.0, seed=None):
    """x0 (rows, D), residual (rows, D) fp32 or None -> out (rows, D) out_dtype, residual' fp32, mean, rstd (rows,).
    ``dropout_p`` > 0: dropout(x0) inside the pass, decided per element from ``seed`` (a one-element int64 tensor on x0's device)."""
    _require_gpu(x0, "x0")
    if dropout_p > 0.0:
        assert seed is not None and seed.dtype == torch.int64 and seed.numel() == 1 and seed.device == x0.device
    rows, D = x0.shape
    out = torch.empty((rows, D), dtype=out_dtype, device=x0.device)
    res_out = torch.empty((rows, D), dtype=torch.float32, device=x0.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x0.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x0.device)
    if rows == 0:
        return out, res_out, mean, rstd
    with _backend.guard(x0.device):
        check(lib().hyena_dropout_add_norm_fwd(x0.data_ptr(), dtype_code(x0.dtype), None if residual is None else residual.data_ptr(),
                                               weight.data_ptr(), bias.data_ptr(), float(eps), float(dropout_p),
                                               seed.data_ptr() if dropout_p > 0.0 else None, out.data_ptr(), dtype_code(out_dtype),
                                               res_out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, D, _backend.stream(x0.device)))
    return out, res_out, mean, rstd


def embed_add_norm_supported(V, D, out_dtype):
    try:
        return bool(lib().hyena_embed_add_norm_supported(int(V), int(D), dtype_code(out_dtype)))
    except TypeError:
        return False


def embed_add_norm_fwd(ids, table, weight, bias, eps, out_dtype, dropout_p=0.0, seed=None):
    """ids (rows,) int64, table (V, D) fp32 -> out (rows, D) out_dtype = LayerNorm(dropout(table[ids])), residual' = dropout(table[ids]) fp32,
    mean, rstd (rows,): the embedding gathered inside the first block's add + LayerNorm pass (include/hyena_block.h)."""
    _require_gpu(table, "table")
    rows, (V, D) = ids.numel(), table.shape
    dev = table.device
    out = torch.empty((rows, D), dtype=out_dtype, device=dev)
    res_out = torch.empty((rows, D), dtype=torch.float32, device=dev)
    mean = torch.empty(rows, dtype=torch.float32, device=dev)
    rstd = torch.empty(rows, dtype=torch.float32, device=dev)
    if rows == 0:
        return out, res_out, mean, rstd
    with _backend.guard(dev):
        check(lib().hyena_embed_add_norm_fwd(ids.data_ptr(), table.data_ptr(), V, weight.data_ptr(), bias.data_ptr(), float(eps),
                                             float(dropout_p), seed.data_ptr() if dropout_p > 0.0 else None, out.data_ptr(),
                                             dtype_code(out_dtype), res_out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, D,
                                             _backend.stream(dev)))
    return out, res_out, mean, rstd


def embed_add_norm_bwd(dout, d_res_out, res_out, ids, V, weight, mean, rstd, dropout_p=0.0, seed=None):
    """-> d_table (V, D) fp32 (per-token-class sums of the gradient of the gathered rows, fixed order), dweight (D,), dbias (D,)."""
    _require_gpu(dout, "dout")
    rows, D = dout.shape
    dev = dout.device
    dt = torch.zeros((V, D), dtype=torch.float32, device=dev)
    dw = torch.zeros(D, dtype=torch.float32, device=dev)
    db = torch.zeros(D, dtype=torch.float32, device=dev)
    if rows == 0:
        return dt, dw, db
    part = torch.empty(lib().hyena_embed_add_norm_partial_floats(rows, D), dtype=torch.float32, device=dev)
    with _backend.guard(dev):
        check(lib().hyena_embed_add_norm_bwd(dout.data_ptr(), dtype_code(dout.dtype), None if d_res_out is None else d_res_out.data_ptr(),
                                             res_out.data_ptr(), ids.data_ptr(), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                             float(dropout_p), seed.data_ptr() if dropout_p > 0.0 else None, dt.data_ptr(), V,
                                             dw.data_ptr(), db.data_ptr(), part.data_ptr(), rows, D, _backend.stream(dev)))
    return dt, dw, db


def soft_embed_add_norm_supported(V, D, out_dtype):
    try:
        return bool(lib().hyena_soft_embed_add_norm_supported(int(V), int(D), dtype_code(out_dtype)))
    except TypeError:
        return False


def _seed_ptr(p, seed, dev):
    if not p > 0.0:
        return None
    assert seed is not None and seed.dtype == torch.int64 and seed.numel() == 1 and seed.device == dev
    return seed.data_ptr()


def soft_embed_add_norm_fwd(ids, table, soft, weight, bias, eps, out_dtype, dropout_p=0.0, seed=None, soft_dropout_p=0.0, soft_seed=None):
    """ids (B, L) int64, table (V, D) fp32, soft (n, D) fp32 with n >= 1 -> out (B (n + L), D) out_dtype, residual' fp32, mean, rstd (B (n + L),):
    the first block's norm over [softdrop(soft) | table[ids]] per batch row, neither the embedding nor the concatenation stored
    (include/hyena_block.h).  Both seeds: one-element int64 tensors on the table's device."""
    _require_gpu(table, "table")
    (B, L), (V, D), n = ids.shape, table.shape, soft.shape[0]
    assert soft.shape == (n, D) and soft.dtype == torch.float32 and table.dtype == torch.float32 and ids.dtype == torch.int64
    if n < 1 or B < 1 or L < 1:
        raise ValueError(f"soft_embed_add_norm_fwd needs at least one soft token, one sequence and one position (got n = {n}, B = {B}, L = {L})")
    dev = table.device
    rows = B * (n + L)
    out = torch.empty((rows, D), dtype=out_dtype, device=dev)
    res_out = torch.empty((rows, D), dtype=torch.float32, device=dev)
    mean = torch.empty(rows, dtype=torch.float32, device=dev)
    rstd = torch.empty(rows, dtype=torch.float32, device=dev)
    with _backend.guard(dev):
        check(lib().hyena_soft_embed_add_norm_fwd(ids.data_ptr(), table.data_ptr(), V, soft.data_ptr(), float(soft_dropout_p),
                                                  _seed_ptr(soft_dropout_p, soft_seed, dev), weight.data_ptr(), bias.data_ptr(), float(eps),
                                                  float(dropout_p), _seed_ptr(dropout_p, seed, dev), out.data_ptr(), dtype_code(out_dtype),
                                                  res_out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, n, L, D, _backend.stream(dev)))
    return out, res_out, mean, rstd


def soft_embed_add_norm_bwd(dout, d_res_out, res_out, weight, mean, rstd, B, n, L, dropout_p=0.0, seed=None, soft_dropout_p=0.0, soft_seed=None):
    """-> d_soft (n, D) fp32: the gradient of the soft tokens alone (frozen backbone), from the B n soft rows of dout / d_res_out / res_out."""
    _require_gpu(dout, "dout")
    rows, D = dout.shape
    assert rows == B * (n + L) and n >= 1
    dev = dout.device
    d_soft = torch.empty((n, D), dtype=torch.float32, device=dev)
    with _backend.guard(dev):
        check(lib().hyena_soft_embed_add_norm_bwd(dout.data_ptr(), dtype_code(dout.dtype), None if d_res_out is None else d_res_out.data_ptr(),
                                                  res_out.data_ptr(), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), float(dropout_p),
                                                  _seed_ptr(dropout_p, seed, dev), float(soft_dropout_p), _seed_ptr(soft_dropout_p, soft_seed, dev),
                                                  d_soft.data_ptr(), B, n, L, D, _backend.stream(dev)))
    return d_soft


def row_head_supported(V, D, dtype):
    try:
        return bool(lib().hyena_row_head_supported(int(V), int(D), dtype_code(dtype)))
    except TypeError:
        return False


def row_head_fwd(x, weight):
    """x (rows, D), weight (V, D), one dtype -> logits (rows, V) of that dtype, each accumulated in an order that does not depend on the row count"""
    _require_gpu(x, "x")
    (rows, D), V = x.shape, weight.shape[0]
    assert weight.shape == (V, D) and weight.dtype == x.dtype and weight.device == x.device
    out = torch.empty((rows, V), dtype=x.dtype, device=x.device)
    if rows:
        with _backend.guard(x.device):
            check(lib().hyena_row_head_fwd(x.data_ptr(), weight.data_ptr(), out.data_ptr(), rows, V, D, dtype_code(x.dtype), _backend.stream(x.device)))
    return out


def row_head_bwd(dy, weight):
    """dy (rows, V), weight (V, D) -> dx (rows, D) = dy weight"""
    _require_gpu(dy, "dy")
    (rows, V), D = dy.shape, weight.shape[1]
    assert weight.shape == (V, D) and weight.dtype == dy.dtype and weight.device == dy.device
    dx = torch.empty((rows, D), dtype=dy.dtype, device=dy.device)
    if rows:
        with _backend.guard(dy.device):
            check(lib().hyena_row_head_bwd(dy.data_ptr(), weight.data_ptr(), dx.data_ptr(), rows, V, D, dtype_code(dy.dtype), _backend.stream(dy.device)))
    return dx


def add_norm_bwd(dout, d_res_out, res_out, weight, mean, rstd, dx_dtype, need_dres, dropout_p=0.0, seed=None, offer_colsum=True):
    """-> dx0 (rows, D) dx_dtype, d_residual_in fp32 or None, dweight (D,), dbias (D,).  (``dropout_p``, ``seed``): the forward's.
    offer_colsum (16-bit dx0): the kernel also sums dx0's columns -- the bias gradient of the linear layer in front of this norm -- and leaves them
    in the side table of ``_gradsum`` for that layer's backward (``colsum`` below asks there first)."""
    _require_gpu(dout, "dout")
    rows, D = dout.shape
    dev = dout.device
    dx = torch.empty((rows, D), dtype=dx_dtype, device=dev)
    dres = torch.empty((rows, D), dtype=torch.float32, device=dev) if need_dres else None
    if rows == 0:
        return dx, dres, torch.zeros(D, dtype=torch.float32, device=dev), torch.zeros(D, dtype=torch.float32, device=dev)
    dw = torch.empty(D, dtype=torch.float32, device=dev)          # (written in full by the fixed-order reduction: no zero fill -- 32 launches per model step)
    db = torch.empty(D, dtype=torch.float32, device=dev)
    part = torch.empty(lib().hyena_add_norm_partial_floats(rows, D), dtype=torch.float32, device=dev)
    from . import _gradsum
    want = offer_colsum and _gradsum.ENABLED and dx_dtype in (torch.bfloat16, torch.float16)
    cs = torch.empty(D, dtype=torch.float32, device=dev) if want else None
    with _backend.guard(dev):
        check(lib().hyena_dropout_add_norm_bwd_colsum(dout.data_ptr(), dtype_code(dout.dtype), None if d_res_out is None else d_res_out.data_ptr(),
                                                      res_out.data_ptr(), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), float(dropout_p),
                                                      seed.data_ptr() if dropout_p > 0.0 else None, dx.data_ptr(), dtype_code(dx_dtype),
                                                      None if dres is None else dres.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                                      None if cs is None else cs.data_ptr(), part.data_ptr(), rows, D, _backend.stream(dev)))
    if want:
        _gradsum.offer(dx, cs)
    return dx, dres, dw, db


# ---- add + LayerNorm + pooled readout of a sequence classifier (include/hyena_block.h, hyena_add_norm_pool_*) ----------
POOL_MODES = {"mean": 0, "sum": 1}


def add_norm_pool_supported(D, x_dtype):
    try:
        return bool(lib().hyena_add_norm_pool_supported(int(D), dtype_code(x_dtype)))
    except TypeError:
        return False


def _pool_lengths(lengths, B, device):
    if lengths is None:
        return None
    assert lengths.dtype == torch.int32 and lengths.shape == (B,) and lengths.device == device and lengths.is_contiguous()
    return lengths


def add_norm_pool_fwd(x0, residual, weight, bias, eps, lengths=None, mode="mean", dropout_p=0.0, seed=None):
    """x0 (B, L, D), residual (B, L, D) fp32 or None, lengths (B,) int32 on x0's device or None -> pooled (B, D) fp32 =
    scale_b * sum_{t < n_b} LayerNorm(dropout(x0) + residual), mean, rstd (B L,): neither the normalised tensor nor residual' is written."""
    _require_gpu(x0, "x0")
    if dropout_p > 0.0:
        assert seed is not None and seed.dtype == torch.int64 and seed.numel() == 1 and seed.device == x0.device
    B, L, D = x0.shape
    dev = x0.device
    lengths = _pool_lengths(lengths, B, dev)
    pooled = torch.zeros((B, D), dtype=torch.float32, device=dev) if B * L == 0 else torch.empty((B, D), dtype=torch.float32, device=dev)
    mean = torch.empty(B * L, dtype=torch.float32, device=dev)
    rstd = torch.empty(B * L, dtype=torch.float32, device=dev)
    if B * L == 0:
        return pooled, mean, rstd
    part = torch.empty(lib().hyena_add_norm_pool_partial_floats(B, L, D) // 3, dtype=torch.float32, device=dev)
    with _backend.guard(dev):
        check(lib().hyena_add_norm_pool_fwd(x0.data_ptr(), dtype_code(x0.dtype), None if residual is None else residual.data_ptr(),
                                            weight.data_ptr(), bias.data_ptr(), float(eps), float(dropout_p),
                                            seed.data_ptr() if dropout_p > 0.0 else None, None if lengths is None else lengths.data_ptr(),
                                            POOL_MODES[mode], pooled.data_ptr(), mean.data_ptr(), rstd.data_ptr(), part.data_ptr(), B, L, D,
                                            _backend.stream(dev)))
    return pooled, mean, rstd


def add_norm_pool_bwd(g, x0, residual, weight, mean, rstd, lengths=None, mode="mean", need_dres=True, dropout_p=0.0, seed=None,
                      offer_colsum=True):
    """g (B, D) fp32, the gradient of pooled -> dx0 (B L, D) x0's dtype, d_residual (B L, D) fp32 or None, dweight (D,), dbias (D,); no
    (B, L, D) dout exists.  offer_colsum: as in add_norm_bwd (the bias gradient of the linear layer in front of this norm)."""
    _require_gpu(g, "g")
    B, L, D = x0.shape
    dev = x0.device
    lengths = _pool_lengths(lengths, B, dev)
    dx = torch.empty((B * L, D), dtype=x0.dtype, device=dev)
    dres = torch.empty((B * L, D), dtype=torch.float32, device=dev) if need_dres else None
    if B * L == 0:
        return dx, dres, torch.zeros(D, dtype=torch.float32, device=dev), torch.zeros(D, dtype=torch.float32, device=dev)
    dw = torch.empty(D, dtype=torch.float32, device=dev)
    db = torch.empty(D, dtype=torch.float32, device=dev)
    part = torch.empty(lib().hyena_add_norm_pool_partial_floats(B, L, D), dtype=torch.float32, device=dev)
    from . import _gradsum
    want = offer_colsum and _gradsum.ENABLED and x0.dtype in (torch.bfloat16, torch.float16)
    cs = torch.empty(D, dtype=torch.float32, device=dev) if want else None
    with _backend.guard(dev):
        check(lib().hyena_add_norm_pool_bwd(g.data_ptr(), x0.data_ptr(), dtype_code(x0.dtype), None if residual is None else residual.data_ptr(),
                                            weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), float(dropout_p),
                                            seed.data_ptr() if dropout_p > 0.0 else None, None if lengths is None else lengths.data_ptr(),
                                            POOL_MODES[mode], dx.data_ptr(), None if dres is None else dres.data_ptr(), dw.data_ptr(),
                                            db.data_ptr(), None if cs is None else cs.data_ptr(), part.data_ptr(), B, L, D,
                                            _backend.stream(dev)))
    if want:
        _gradsum.offer(dx, cs)
    return dx, dres, dw, db

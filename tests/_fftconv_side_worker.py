"""Child process of tests/test_gpu_fftconv_local.py::test_side_stream_off: started with HYENA_FFTCONV_SIDE=0 (the library reads the knob once per
process), computes tests.fftconv_local.side_case_outputs for fp32 and bf16 on the GPU and writes them to the file named on the command line."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hyena_dna_amd import _lib  # noqa: E402
from tests import fftconv_local as FL  # noqa: E402

if __name__ == "__main__":
    assert os.environ.get("HYENA_FFTCONV_SIDE") == "0" and torch.cuda.is_available() and _lib._backend.name == "hip"
    dev = torch.device("cuda", 0)
    res = {FL.NAME[T]: FL.side_case_outputs(_lib, dev, T) for T in FL.E_TYPES}
    torch.cuda.synchronize()
    torch.save(res, sys.argv[1])
    print("SIDE_OFF_OK")

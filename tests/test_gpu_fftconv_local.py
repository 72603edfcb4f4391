"""MI355X: the long convolution of the gfx950 library against the element-wise fp64 references and bounds of tests/fftconv_local.py, every
kernel branch reached by design and every case asserting the kernels it reaches: the two-level column kernels of all 30 column sizes in all
three types (A), the row kernels and the host loop over channel chunks (B), the workspace-free plan under every knob (C), pitched rows with
guards (D) and the side stream switched off in a fresh process (E).  The suites are those of tests/test_fftconv_local_emu.py, which has no E.
Figures and run times: profiles/fftconv_local.md."""
import os
import subprocess
import sys

import pytest
import torch

from tests import fftconv_local as FL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = FL.NAME.get


def _dev():
    return torch.device("cuda", 0)


_A = [(M1, kind, T) for M1, kind in FL.A_PARAMS for T in FL.DTYPES if kind == "ragged" or T != FL.F16]


@pytest.mark.parametrize("M1,kind,dtype", _A, ids=lambda v: FL.NAME[v] if isinstance(v, torch.dtype) else str(v))
def test_column_kernels(gpu_lib, monkeypatch, M1, kind, dtype):
    FL.suite_columns(gpu_lib, _dev(), monkeypatch, dtype, M1, kind, "gpu")


@pytest.mark.parametrize("i", range(len(FL.B_CASES)), ids=lambda i: "M1_{}-B{}-chunk{}-need{}{}-saved{}-bias{}-{}".format(
    *FL.B_CASES[i][:3], *FL.B_CASES[i][3], *FL.B_CASES[i][4:6], FL.NAME[FL.B_CASES[i][6]]))
def test_row_kernels_and_host_loop(gpu_lib, monkeypatch, i):
    FL.suite_rows(gpu_lib, _dev(), monkeypatch, i, "gpu")


_C = [(i, T) for i, c in enumerate(FL.C_CASES) for T in c[7]]


@pytest.mark.parametrize("i,dtype", _C, ids=lambda v: FL.NAME[v] if isinstance(v, torch.dtype) else "c{}-R{}-B{}-D{}-L{}".format(v, *FL.C_CASES[v][:4]))
def test_workspace_free_plan(gpu_lib, monkeypatch, i, dtype):
    FL.suite_onchip(gpu_lib, _dev(), monkeypatch, i, dtype, "gpu")


@pytest.mark.parametrize("dtype", [FL.F32, FL.BF16], ids=ids)
@pytest.mark.parametrize("i", range(len(FL.C_PROBES)))
def test_workspace_free_probes(gpu_lib, monkeypatch, i, dtype):
    FL.suite_onchip_probes(gpu_lib, _dev(), monkeypatch, i, dtype, "gpu")


@pytest.mark.parametrize("dtype", [FL.F32, FL.BF16], ids=ids)
@pytest.mark.parametrize("i", range(len(FL.D_CASES)))
def test_pitched_rows_with_guards(gpu_lib, monkeypatch, i, dtype):
    FL.suite_pitched(gpu_lib, _dev(), monkeypatch, i, dtype, "gpu")


def test_side_stream_off(gpu_lib, monkeypatch, tmp_path):
    """HYENA_FFTCONV_SIDE=0 -- also what a process runs whose side stream cannot be created: the self-paired rows on the caller's stream.  One
    child process (the knob is read once per process), M1 = 64, B = 2, fp32 and bf16: the same bits as this process computes with the side
    stream on, which tables A and B hold to the reference."""
    B, D, L, want = FL.E_CASE
    path = str(tmp_path / "side_off.pt")
    env = dict(os.environ, HYENA_FFTCONV_SIDE="0")
    for name in FL.KNOBS:
        env.pop(name, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_fftconv_side_worker.py"), path], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-1500:], p.stderr[-2500:])
    assert "SIDE_OFF_OK" in p.stdout
    child = torch.load(path)
    assert os.environ.get("HYENA_FFTCONV_SIDE", "1")[:1] != "0", "this process must run with the side stream on"
    with FL.knobs(monkeypatch, None):
        assert FL.route(gpu_lib, B, D, L) == want
        for T in FL.E_TYPES:
            mine = FL.side_case_outputs(gpu_lib, _dev(), T)
            for name, a, c in zip(("out", "du", "dk", "dbias"), mine, child[FL.NAME[T]]):
                assert FL.same_bits(a, c), (name, FL.NAME[T], "the side stream changes the bits")

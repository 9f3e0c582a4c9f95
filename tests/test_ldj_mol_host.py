"""CPU-only checks of the per-molecule log-density entries: the reverse pass's
log|detJ| (enflow_lf_reverse_io3_f32, enflow_lf_reverse_large_ldj_f32) and the
per-molecule negative log-likelihood (enflow_alchemical_nll_mol_f32) are
exported by both libraries with ctypes signatures, the ABI version stays 13,
argument errors return their code without launching anything, and the Python
surface refuses CPU tensors and autograd."""
import ctypes

import pytest
import torch

from enflow_amd import _lib
from enflow_amd.data.synthetic import make_molecules, default_dt

NEW = ("enflow_lf_reverse_io3_f32", "enflow_lf_reverse_large_ldj_f32", "enflow_alchemical_nll_mol_f32")


@pytest.mark.parametrize("nf", [None, 16], ids=["libenflow_hip", "libenflow_hip_nf16"])
def test_new_entries_exported_with_signatures(nf):
    L = _lib.lib(nf)
    assert L.enflow_abi_version() == 13      # additive exports only
    for name in NEW:
        assert hasattr(L, name), name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    # the io2 / large reverse arguments plus the new ones, before the stream
    assert len(_lib.SIGNATURES["enflow_lf_reverse_io3_f32"][1]) == len(_lib.SIGNATURES["enflow_lf_reverse_io2_f32"][1]) + 3
    assert len(_lib.SIGNATURES["enflow_lf_reverse_large_ldj_f32"][1]) == \
        len(_lib.SIGNATURES["enflow_lf_reverse_large_f32"][1]) + 2


# never dereferenced: every call below is refused before a launch (or has nothing to launch)
_BUF = ctypes.create_string_buffer(64)
P = ctypes.addressof(_BUF)


def _io3(num_mols=1, max_n=20, nf=5, hid=128, n_layers=1, kind=0, prec=1, outs=(P, P, P, P), idx=(None, None),
         err=P, mol_list=None, num_listed=0, ldj_mol=P, ldj_total=None, ticket=None):
    return [num_mols, num_mols * max_n, max_n, nf, hid, P, P, P, None, None, None, None, *outs, P, n_layers,
            kind, 0.1, 1.0, *idx, err, prec, None, mol_list, num_listed, ldj_mol, ldj_total, ticket, None]


@pytest.mark.parametrize("nf_lib,nfmax", [(None, 8), (16, 16)], ids=["libenflow_hip", "libenflow_hip_nf16"])
def test_reverse_io3_argument_errors_launch_nothing(nf_lib, nfmax):
    f = _lib.lib(nf_lib).enflow_lf_reverse_io3_f32
    assert f(*_io3(ldj_mol=None)) == -1                      # ldj_mol is required
    assert f(*_io3(ldj_total=P)) == -1                       # ldj_total and ticket: both or neither
    assert f(*_io3(ticket=P)) == -1
    assert f(*_io3(mol_list=P, num_listed=1, ldj_total=P, ticket=P)) == -1   # a molecule list takes no ticket
    assert f(*_io3(mol_list=P, num_listed=2)) == -1          # more listed than molecules
    assert f(*_io3(num_mols=-1)) == -1
    assert f(*_io3(nf=0)) == -4 and f(*_io3(nf=nfmax + 1)) == -4
    assert f(*_io3(hid=96)) == -5
    assert f(*_io3(max_n=300)) == -3
    assert f(*_io3(prec=7)) == -1
    assert f(*_io3(n_layers=-1)) == -1
    assert f(*_io3(outs=(P, None, P, P))) == -1
    assert f(*_io3(err=None)) == -1
    assert f(*_io3(kind=_lib.DEQUANT_ARGMAX)) == -1          # ArgMax without its index outputs
    assert f(*_io3(num_mols=0)) == 0                         # nothing to do
    assert f(*_io3(num_mols=0, ldj_total=P, ticket=P)) == 0


@pytest.mark.parametrize("nf_lib,nfmax", [(None, 8), (16, 16)], ids=["libenflow_hip", "libenflow_hip_nf16"])
def test_reverse_large_ldj_argument_errors_launch_nothing(nf_lib, nfmax):
    L = _lib.lib(nf_lib)
    f = L.enflow_lf_reverse_large_ldj_f32
    need = L.enflow_lf_large_workspace_size(1, 300, 300, 5)

    def args(num_mols=1, nf=5, hid=128, prec=1, ws=P, ws_bytes=None, ldj_mol=P, ldj_total=P, err=P, kind=0):
        return [num_mols, 300 * max(num_mols, 0), 300, nf, hid, P, P, P, P, P, P, P, P, 1, kind, 0.1, 1.0,
                None, None, err, prec, ws, need if ws_bytes is None else ws_bytes, ldj_mol, ldj_total, None]

    assert f(*args(ldj_mol=None)) == -1
    assert f(*args(ldj_total=None)) == -1
    assert f(*args(ws=None)) == -1
    assert f(*args(err=None)) == -1
    assert f(*args(kind=_lib.DEQUANT_ARGMAX)) == -1
    assert f(*args(num_mols=-1)) == -1
    assert f(*args(nf=0)) == -4 and f(*args(nf=nfmax + 1)) == -4
    assert f(*args(hid=96)) == -5
    assert f(*args(prec=7)) == -1
    assert f(*args(ws_bytes=need - 1)) == -6
    assert f(*args(num_mols=0)) == 0


@pytest.mark.parametrize("nf_lib", [None, 16], ids=["libenflow_hip", "libenflow_hip_nf16"])
def test_nll_mol_argument_errors_launch_nothing(nf_lib):
    f = _lib.lib(nf_lib).enflow_alchemical_nll_mol_f32
    good = [1, P, P, P, 1.0, 10.0, P, None]
    for i in (1, 2, 3, 6):          # mol_ptr, nll_mol, ldj_mol, out
        bad = list(good)
        bad[i] = None
        assert f(*bad) == -1, i
    assert f(*([-1] + good[1:])) == -1
    assert f(*([0] + good[1:])) == 0


def _cpu_flow(trainable):
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data import Data
    torch.manual_seed(0)
    model = LFIntegrator([EGCL(5, 5, 32) for _ in range(2)], ArgMax(5, 32), dt=default_dt())
    for p in model.parameters():
        p.requires_grad_(trainable)
    return model, Data.from_arrays(make_molecules(2, [3, 4], seed=0), device="cpu")


def test_python_surface_refuses_cpu_tensors():
    from enflow_amd.flow import Alchemical_NLL
    model, d = _cpu_flow(False)
    with pytest.raises(_lib.HipPathError):
        model.reverse(d, return_ldj=True)
    with pytest.raises(_lib.HipPathError):
        model.forward(d, per_molecule=True)
    nll = Alchemical_NLL(kBT=1.0)
    with pytest.raises(_lib.HipPathError):
        nll.per_molecule(d, torch.zeros(2))
    with pytest.raises(_lib.HipPathError):
        nll.potential(d)


def test_autograd_is_refused_and_names_no_grad():
    """Inference only: a flow with a trainable parameter (grad enabled), and a
    loss input that requires grad, raise NotImplementedError naming
    torch.no_grad() before anything touches the device."""
    model, d = _cpu_flow(True)
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\)"):
        model.reverse(d, return_ldj=True)
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\)"):
        model.forward(d, per_molecule=True)
    with torch.no_grad():            # the same flow under no_grad gets as far as the device check
        with pytest.raises(_lib.HipPathError):
            model.reverse(d, return_ldj=True)


def test_loss_autograd_is_refused(monkeypatch):
    from enflow_amd.flow import Alchemical_NLL
    _, d = _cpu_flow(False)
    monkeypatch.setattr(_lib, "require_gpu", lambda t: None)     # reach the autograd check on a CPU machine
    nll = Alchemical_NLL(kBT=1.0)
    d.pos = d.pos.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\)"):
        nll.per_molecule(d, torch.zeros(2))
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\)"):
        nll.potential(d)
    d.pos = d.pos.detach()
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\)"):
        nll.per_molecule(d, torch.zeros(2, requires_grad=True))

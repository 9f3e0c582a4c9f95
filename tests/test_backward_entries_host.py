"""CPU-only table of the training backward's C entries and the code each argument
error returns (enflow_lf_backward_f32, enflow_lf_backward_large_f32,
enflow_egcl_backward_f32, enflow_egcl_backward_large_f32,
enflow_lf_reverse_backward_f32, enflow_argmax_backward_f32 and the
*_workspace_size beside each), on both libraries.

Every case returns before the entry's first HIP call, so nothing is launched and
no pointer is dereferenced: pointers are the never-read address 8.  The standalone
EGCL entries zero a workspace word (hipMemsetAsync) once their own checks pass,
so their table stops at those checks: the empty batch is not among their cases and
a pair_row_bound of 2^31 is only seen with a workspace that is too small.

The expected codes are literals recorded from the library before its host half
was rewritten around BwdCall / AuxPipe; a disagreement is a regression."""
import pytest

from enflow_amd import _lib

P = 8            # a non-null pointer that is never dereferenced
BIG = 1 << 60    # workspace_bytes that is always enough

# name -> (argument names in the header's order, {argument: value of a good call})
_SIZES = dict(num_mols=3, num_atoms=58, max_mol_atoms=33, nf=5, H=32, n_layers=3, pair_row_bound=4096,
              workspace_bytes=BIG, dt=0.01, cw=1.0, stream=None)
ENTRIES = {
    "enflow_lf_backward_f32": (
        "num_mols num_atoms max_mol_atoms nf H mol_ptr r_cut box tape pair_counts layers layers_bwd layers_raw "
        "n_layers dequant_kind dequant_raw h_data noise dt cw adj_h adj_g adj_pos adj_vel adj_ldj grad_layers "
        "grad_dequant workspace workspace_bytes pair_row_bound err_flag stream",
        dict(dequant_kind=_lib.DEQUANT_ARGMAX)),
    "enflow_lf_backward_large_f32": (
        "num_mols num_atoms max_mol_atoms nf H mol_ptr r_cut box tape layers layers_bwd layers_raw "
        "n_layers dequant_kind dequant_raw h_data noise dt cw adj_h adj_g adj_pos adj_vel adj_ldj grad_layers "
        "grad_dequant workspace workspace_bytes pair_row_bound err_flag stream",
        dict(dequant_kind=_lib.DEQUANT_ARGMAX, max_mol_atoms=65)),
    "enflow_egcl_backward_f32": (
        "num_mols num_atoms max_mol_atoms nf H mol_ptr r_cut box tape pair_counts layer layer_bwd layer_raw "
        "egcl_flags cw adj_Q adj_F adj_G adj_h adj_pos grad_layer workspace workspace_bytes pair_row_bound "
        "err_flag stream",
        dict(egcl_flags=0)),
    "enflow_egcl_backward_large_f32": (
        "num_mols num_atoms max_mol_atoms nf H mol_ptr r_cut box tape layer layer_bwd layer_raw "
        "egcl_flags cw adj_Q adj_F adj_G adj_h adj_pos grad_layer workspace workspace_bytes pair_row_bound "
        "err_flag stream",
        dict(egcl_flags=0, max_mol_atoms=65)),
    "enflow_lf_reverse_backward_f32": (
        "num_mols num_atoms max_mol_atoms nf H mol_ptr r_cut box state_h state_pos state_vel layers layers_bwd "
        "layers_raw n_layers flags gemm_precision dt cw adj_h adj_g adj_pos adj_vel adj_ldj grad_layers workspace "
        "workspace_bytes pair_row_bound err_flag stream",
        dict(flags=0, gemm_precision=_lib.PREC_F16X3)),
    "enflow_argmax_backward_f32": (
        "num_mols num_atoms max_mol_atoms nf H mol_ptr h dequant_raw noise adj_z adj_log_q grad_dequant workspace "
        "workspace_bytes stream",
        dict()),
}


def call(L, name, **over):
    names, good = ENTRIES[name]
    vals = {**_SIZES, **good, **over}
    assert set(over) <= set(names.split()), (name, over)
    return getattr(L, name)(*[vals.get(a, P) for a in names.split()])


def need(L, name, **over):
    """The entry's smallest accepted workspace_bytes at the good call's sizes."""
    v = {**_SIZES, **ENTRIES[name][1], **over}
    M, A, n, nf, H, nl, prb = (v[k] for k in ("num_mols", "num_atoms", "max_mol_atoms", "nf", "H", "n_layers",
                                              "pair_row_bound"))
    return {
        "enflow_lf_backward_f32": lambda: L.enflow_lf_backward_workspace_size_min(M, A, nf, H, nl, prb),
        "enflow_lf_backward_large_f32": lambda: L.enflow_lf_backward_large_workspace_size(M, A, n, nf, H, prb),
        "enflow_egcl_backward_f32": lambda: L.enflow_egcl_backward_workspace_size(M, A, nf, H, prb),
        "enflow_egcl_backward_large_f32": lambda: L.enflow_egcl_backward_large_workspace_size(M, A, n, nf, H, prb),
        "enflow_lf_reverse_backward_f32": lambda: L.enflow_lf_reverse_backward_workspace_size(M, A, n, nf, H, prb),
        "enflow_argmax_backward_f32": lambda: L.enflow_argmax_backward_workspace_size(A, nf, H),
    }[name]()


WIDE = "nf past the library's limit"   # replaced by enflow_max_node_nf() + 1
FUSED = ("enflow_lf_backward_f32", "enflow_lf_backward_large_f32")
EGCL = ("enflow_egcl_backward_f32", "enflow_egcl_backward_large_f32")
REV = ("enflow_lf_reverse_backward_f32",)
AM = ("enflow_argmax_backward_f32",)
PRB = FUSED + EGCL + REV   # entries with a pair_row_bound
# (entries, overrides of the good call, the code returned)
TABLE = [
    (PRB + AM, dict(num_mols=-1), -1),
    (PRB + AM, dict(num_atoms=-1), -1),
    (FUSED + EGCL[1:] + REV + AM, dict(max_mol_atoms=-1), -1),
    (EGCL[:1], dict(max_mol_atoms=-1, workspace_bytes=0), -6),   # not looked at before the workspace
    (FUSED[:1] + AM, dict(max_mol_atoms=65), -1),
    (FUSED[1:] + EGCL[1:] + REV, dict(max_mol_atoms=1 << 22), -1),
    (PRB + AM, dict(nf=0), -1),
    (PRB + AM, dict(nf=WIDE), -1),
    (PRB + AM, dict(H=48), -1),
    (PRB + AM, dict(H=256), -1),
    (FUSED + REV, dict(n_layers=-1), -1),
    (PRB, dict(pair_row_bound=-1), -1),
    (FUSED + EGCL[1:] + REV, dict(pair_row_bound=1 << 31), -1),
    (EGCL[:1], dict(pair_row_bound=1 << 31, workspace_bytes=0), -6),   # its int32 check follows the memset
    (REV, dict(gemm_precision=_lib.PREC_BF16), -1),
    (REV, dict(gemm_precision=3), -1),
    # a null required pointer
    (FUSED + EGCL + REV, dict(workspace=None), -1),
    (FUSED + EGCL, dict(tape=None, workspace_bytes=0), (-1, -1, -6, -6)),
    (FUSED[:1], dict(pair_counts=None), -1),
    (FUSED[1:], dict(mol_ptr=None), -1),
    (FUSED + REV, dict(layers_raw=None), -1),
    (FUSED + REV, dict(adj_ldj=None), -1),
    (FUSED + REV, dict(grad_layers=None), -1),
    (FUSED + REV, dict(err_flag=None), -1),
    (FUSED, dict(grad_dequant=None), -1),                       # ArgMax dequantiser: its four pointers
    (FUSED, dict(noise=None), -1),
    (EGCL, dict(adj_Q=None), -1),
    (EGCL, dict(adj_G=None), -1),
    (REV, dict(state_vel=None), -1),
    (AM, dict(adj_log_q=None), -1),
    (AM, dict(workspace=None), -1),
    # argument errors come before the workspace size
    (PRB + AM, dict(nf=0, workspace_bytes=0), -1),
    (EGCL, dict(adj_F=None, workspace_bytes=0), -1),
    # the empty batch: after the checks, before anything is launched
    (FUSED + REV + AM, dict(num_mols=0), 0),
    (FUSED + REV + AM, dict(num_mols=0, workspace=None), -1),
    (FUSED + REV + AM, dict(num_mols=0, workspace_bytes=0), -6),
    (REV, dict(num_atoms=0), 0),
    (REV, dict(n_layers=0), 0),
]


@pytest.fixture(params=[None, 16], ids=["libenflow_hip", "libenflow_hip_nf16"])
def L(request):
    return _lib.lib(request.param)


def test_argument_errors_return_their_codes_before_any_launch(L):
    assert L.enflow_abi_version() == 13
    width = L.enflow_max_node_nf()
    for names, over, want in TABLE:
        over = {k: (width + 1 if v is WIDE else v) for k, v in over.items()}
        wants = want if isinstance(want, tuple) else (want,) * len(names)
        for name, w in zip(names, wants):
            assert call(L, name, **over) == w, (name, over, w)
    for name in ENTRIES:   # the library's widest nf is accepted (it fails on a later argument)
        assert call(L, name, nf=width, workspace=None) == -1 and call(L, name, nf=width, workspace_bytes=0) == -6


def test_workspace_one_byte_short_is_minus_6(L):
    for name in ENTRIES:
        n = need(L, name)
        assert n > 0, name
        assert call(L, name, workspace_bytes=n - 1) == -6, name
        assert call(L, name, workspace_bytes=0) == -6, name
    # the fused flow takes the two-buffer size; three buffers are larger from three layers on
    full = L.enflow_lf_backward_workspace_size(3, 58, 5, 32, 3, 4096)
    lean = L.enflow_lf_backward_workspace_size_min(3, 58, 5, 32, 3, 4096)
    assert lean < full
    assert call(L, "enflow_lf_backward_f32", num_mols=0, workspace_bytes=lean) == 0   # enough: the empty batch returns


def test_workspace_sizes_refuse_bad_arguments(L):
    width = L.enflow_max_node_nf()
    lf, lf_min = L.enflow_lf_backward_workspace_size, L.enflow_lf_backward_workspace_size_min
    for size in (lf, lf_min):          # (num_mols, num_atoms, nf, H, n_layers, pair_row_bound)
        assert size(3, 58, 5, 32, 3, 4096) > 0 and size(0, 0, 5, 32, 0, 0) >= 0
        for bad in ((-1, 58, 5, 32, 3, 4096), (3, -1, 5, 32, 3, 4096), (3, 58, 0, 32, 3, 4096),
                    (3, 58, width + 1, 32, 3, 4096), (3, 58, 5, 48, 3, 4096), (3, 58, 5, 32, -1, 4096),
                    (3, 58, 5, 32, 3, -1)):
            assert size(*bad) == -1, bad
        assert size(3, 58, width, 32, 3, 4096) > 0
        assert size(3, 58, 5, 32, 3, 1 << 31) > 0      # the size is defined past int32 rows; the entry refuses them
    # (num_mols, num_atoms, max_mol_atoms, nf, H, pair_row_bound)
    for size in (L.enflow_lf_backward_large_workspace_size, L.enflow_egcl_backward_large_workspace_size,
                 L.enflow_lf_reverse_backward_workspace_size):
        assert size(3, 58, 65, 5, 32, 4096) > 0 and size(3, 58, 65, width, 32, 4096) > 0
        for bad in ((-1, 58, 65, 5, 32, 4096), (3, -1, 65, 5, 32, 4096), (3, 58, -1, 5, 32, 4096),
                    (3, 58, 1 << 22, 5, 32, 4096), (3, 58, 65, 0, 32, 4096), (3, 58, 65, width + 1, 32, 4096),
                    (3, 58, 65, 5, 48, 4096), (3, 58, 65, 5, 32, -1), (3, 58, 65, 5, 32, 1 << 31)):
            assert size(*bad) == -1, bad
    assert L.enflow_lf_reverse_backward_workspace_size(3, 58, 33, 5, 32, 4096) > 0     # its fused branch
    eg = L.enflow_egcl_backward_workspace_size          # (num_mols, num_atoms, nf, H, pair_row_bound)
    assert eg(3, 58, 5, 32, 4096) > lf(3, 58, 5, 32, 1, 4096) and eg(3, 58, width, 32, 4096) > 0
    for bad in ((-1, 58, 5, 32, 4096), (3, -1, 5, 32, 4096), (3, 58, 0, 32, 4096), (3, 58, width + 1, 32, 4096),
                (3, 58, 5, 48, 4096), (3, 58, 5, 32, -1)):
        assert eg(*bad) == -1, bad
    am = L.enflow_argmax_backward_workspace_size        # (num_atoms, nf, H)
    assert am(58, 5, 32) > 0 and am(0, 5, 32) == 0 and am(58, width, 32) > 0
    for bad in ((-1, 5, 32), (58, 0, 32), (58, width + 1, 32), (58, 5, 48)):
        assert am(*bad) == -1, bad

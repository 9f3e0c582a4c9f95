"""CPU-only checks of the edge-list EGCL's host side: enflow_egcl_forward_list_f32
is declared in include/enflow_hip.h, bound with the header's argument count and
exported by both libraries without an ABI bump; every argument error returns
its code before any launch; CPU tensors and objects that are no edge list are
refused."""
import os
import re

import pytest
import torch

from enflow_amd import _lib
from enflow_amd.nn import EGCL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "enflow_hip.h")
NAME = "enflow_egcl_forward_list_f32"


def header_prototypes():
    """{name: number of parameters} of every prototype in the header."""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(enflow_\w+)\s*\(([^)]*)\)\s*;", txt):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_entry_declared_and_bound_with_the_headers_argument_count():
    protos = header_prototypes()
    assert NAME in protos, f"{NAME} is not declared in include/enflow_hip.h"
    assert NAME in _lib.SIGNATURES, f"{NAME} has no ctypes signature"
    assert len(_lib.SIGNATURES[NAME][1]) == protos[NAME] == 16
    assert re.search(r"#define\s+ENFLOW_ERR_INDEX\s+64\b", open(HEADER).read())
    assert _lib.ERR_INDEX == 64


def call(L, n=49, E=100, nf=5, H=128, prec=_lib.PREC_F32):
    """The entry with every pointer null: whatever it returns, it launched nothing."""
    return L.enflow_egcl_forward_list_f32(n, E, nf, H, None, None, None, None, None, 1.0, None, None, None, None,
                                          prec, None)


@pytest.mark.parametrize("nf", [None, 16], ids=["libenflow_hip", "libenflow_hip_nf16"])
def test_entry_exported_and_argument_errors_launch_nothing(nf):
    L = _lib.lib(nf)
    assert L.enflow_abi_version() == 13   # additive export: no ABI bump
    assert hasattr(L, NAME)
    width = L.enflow_max_node_nf()
    assert call(L) == -1                                   # null pointers
    assert call(L, n=-1) == -1 and call(L, E=-1) == -1     # negative sizes
    assert call(L, prec=_lib.PREC_BF16) == -1              # bf16 has no instance
    assert call(L, prec=3) == -1 and call(L, prec=_lib.PREC_NO_SPLIT) == -1
    assert call(L, prec=_lib.PREC_F16X3 | _lib.EGCL_VARIANTS) == -1   # a known precision: on to the pointers
    assert call(L, nf=0) == -4 and call(L, nf=width + 1) == -4
    assert call(L, nf=width) == -1
    assert call(L, H=48) == -5 and call(L, H=256) == -5
    for H in (32, 64, 128):
        assert call(L, H=H) == -1
    assert call(L, n=(1 << 22) + 1) == -3                  # the pair words' 22-bit column field
    assert call(L, n=1 << 22) == -1
    assert call(L, E=(1 << 31) - 1024) == -3               # int32 row_ptr
    assert call(L, n=0, E=0) == -1                         # null pointers come before the empty batch


class List:
    def __init__(self, row, col, coord_diff):
        self.row, self.col, self.coord_diff = row, col, coord_diff


def test_cpu_tensors_are_refused():
    net = EGCL(5, 5, 32)
    h = torch.zeros((3, 5))
    edges = List(torch.tensor([0, 1]), torch.tensor([1, 2]), torch.zeros((2, 3)))
    with torch.no_grad(), pytest.raises(_lib.HipPathError):
        net(h, edges)
    with pytest.raises(_lib.HipPathError):
        net._infer_list(h, edges.row, edges.col, edges.coord_diff)


def test_objects_that_are_no_edge_list_raise_type_error():
    net = EGCL(5, 5, 32)
    h = torch.zeros((3, 5))

    class NoDiff:
        row = torch.tensor([0])
        col = torch.tensor([1])

    for bad in (None, (torch.tensor([0]), torch.tensor([1])), NoDiff(), torch.zeros((2, 1), dtype=torch.long)):
        with torch.no_grad(), pytest.raises(TypeError):
            net(h, bad)

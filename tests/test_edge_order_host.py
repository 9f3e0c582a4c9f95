"""CPU-only checks of the explicit edge list's host side: the entry points are
declared in include/enflow_hip.h, bound with matching argument counts and
exported by both libraries; argument errors launch nothing; CPU tensors are
refused like everywhere else."""
import os
import re

import pytest
import torch

from enflow_amd import _lib
from enflow_amd.data import Data
from enflow_amd.data.base import Edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "enflow_hip.h")
NEW = ("enflow_edge_list_workspace_size", "enflow_edge_list_count_f32", "enflow_edge_list_fill_f32")


def header_prototypes():
    """{name: number of parameters} of every prototype in the header."""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(enflow_\w+)\s*\(([^)]*)\)\s*;", txt):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_entries_declared_and_bound_with_matching_argument_counts():
    protos = header_prototypes()
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/enflow_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert len(_lib.SIGNATURES[name][1]) == protos[name], name
    assert len(_lib.SIGNATURES["enflow_edge_list_count_f32"][1]) == 11
    assert len(_lib.SIGNATURES["enflow_edge_list_fill_f32"][1]) == 15


@pytest.mark.parametrize("nf", [None, 16], ids=["libenflow_hip", "libenflow_hip_nf16"])
def test_entries_exported_and_argument_errors_launch_nothing(nf):
    L = _lib.lib(nf)
    assert L.enflow_abi_version() == 13   # additive exports: no ABI bump
    for name in NEW:
        assert hasattr(L, name), name
    assert L.enflow_edge_list_workspace_size(-1, 0) == -1
    assert L.enflow_edge_list_workspace_size(0, -1) == -1
    small, big = L.enflow_edge_list_workspace_size(1, 22), L.enflow_edge_list_workspace_size(3, 2944)
    assert 22 * 27 * 12 <= small < big   # cnt (int32) and off (int64) per (atom, shift)
    # null workspace / outputs, negative sizes: -1 before any launch (no GPU here)
    assert L.enflow_edge_list_count_f32(1, 22, None, None, None, None, None, None, None, 0, None) == -1
    assert L.enflow_edge_list_count_f32(-1, 0, None, None, None, None, None, None, None, 0, None) == -1
    assert L.enflow_edge_list_fill_f32(1, 22, None, None, None, None, None, 5, None, None, None, None,
                                       None, 0, None) == -1
    assert L.enflow_edge_list_fill_f32(1, 22, None, None, None, None, None, -1, None, None, None, None,
                                       None, 0, None) == -1


def test_cpu_tensors_are_refused():
    pos = torch.zeros((3, 3))
    e = Edges(pos, torch.full((3, 3), 2.0), torch.tensor([0.9]), torch.tensor([3]))
    with pytest.raises(_lib.HipPathError):
        e.edge_index
    with pytest.raises(_lib.HipPathError):
        e.reference()
    d = Data(h=torch.zeros((3, 5)), g=torch.zeros((3, 5)), pos=pos, vel=torch.zeros((3, 3)), N=torch.tensor([3]),
             r_cut=torch.tensor([0.9]), box=torch.full((3, 3), 2.0))
    with pytest.raises(_lib.HipPathError):
        d.edges.edge_index

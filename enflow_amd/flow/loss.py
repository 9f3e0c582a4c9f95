"""Alchemical negative log-likelihood (mirrors enflow/flow/loss.py:5-24).

__call__(out, ldj) -> 0-d tensor, computed by enflow_alchemical_nll_f32: one
workgroup per molecule sums the softened LJ energy over i < j pairs (zero
distances dropped, loss.py:14-18), sum vel^2, h^2, g^2; a fixed-order double
reduction forms the reference's scalar.  When its inputs carry autograd
history the loss is differentiable (backward: enflow_alchemical_nll_backward_f32).

per_molecule(out, ldj_mol) and potential(out) return the same pieces for each
molecule on its own ([num_mols] tensors; inference only): what a caller needs
to reweight generated configurations.  per_molecule_grad / potential_grad are
the same values with a grad_fn that takes a per-molecule upstream gradient
(backward: enflow_alchemical_nll_mol_backward_f32): training by energy, with
every molecule weighted on its own.
"""
import torch

from .. import _lib
from ..utils.helpers import batch_meta


class Alchemical_NLL:
    def __init__(self, kBT, partition_func=10, softening=0):
        self.kBT = kBT
        self.z_lj = partition_func
        self.softening = softening

    def __call__(self, out, ldj):
        _lib.require_gpu(out.pos)
        if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                           for t in (out.h, out.g, out.pos, out.vel, ldj)):
            return self._differentiable(out, ldj)
        L = _lib.lib(out.h.shape[1])
        dev = out.pos.device
        f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
        h, g, pos, vel = f(out.h), f(out.g), f(out.pos), f(out.vel)
        ptr, max_n = batch_meta(out, dev)
        M = ptr.numel() - 1
        ldj_t = torch.as_tensor(ldj, device=dev).to(torch.float32).reshape(1).contiguous()
        nll_mol = torch.empty((max(M, 1), 4), dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        _lib.check(L.enflow_alchemical_nll_f32(M, h.shape[0], max_n, h.shape[1], _lib.ptr(ptr),
                                               _lib.ptr(h), _lib.ptr(g), _lib.ptr(pos), _lib.ptr(vel),
                                               _lib.ptr(ldj_t), float(self.kBT), float(self.softening),
                                               float(self.z_lj), _lib.ptr(nll_mol), _lib.ptr(loss),
                                               _lib.stream_ptr(dev)), "enflow_alchemical_nll_f32")
        return loss.reshape(()).to(out.h.dtype)

    def _nll_mol(self, out, what):
        """(nll_mol [M][4], mol_ptr, M, device): enflow_alchemical_nll_f32's per-molecule rows."""
        _lib.require_gpu(out.pos)
        if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                           for t in (out.h, out.g, out.pos, out.vel)):
            raise NotImplementedError(f"Alchemical_NLL.{what} is inference-only (the HIP backward takes the "
                                      f"batch scalar): call it under torch.no_grad(), or Alchemical_NLL.{what}_grad")
        L = _lib.lib(out.h.shape[1])
        dev = out.pos.device
        f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
        h, g, pos, vel = f(out.h), f(out.g), f(out.pos), f(out.vel)
        ptr, max_n = batch_meta(out, dev)
        M = ptr.numel() - 1
        zero = torch.zeros(1, dtype=torch.float32, device=dev)
        nll_mol = torch.empty((max(M, 1), 4), dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        _lib.check(L.enflow_alchemical_nll_f32(M, h.shape[0], max_n, h.shape[1], _lib.ptr(ptr),
                                               _lib.ptr(h), _lib.ptr(g), _lib.ptr(pos), _lib.ptr(vel),
                                               _lib.ptr(zero), float(self.kBT), float(self.softening),
                                               float(self.z_lj), _lib.ptr(nll_mol), _lib.ptr(loss),
                                               _lib.stream_ptr(dev)), "enflow_alchemical_nll_f32")
        return nll_mol, ptr, M, dev

    def potential(self, out):
        """The softened LJ energy of each molecule (loss.py:11-19), ``[num_mols]``."""
        nll_mol, _, M, _ = self._nll_mol(out, "potential")
        return nll_mol[:M, 0].contiguous().to(out.h.dtype)

    def per_molecule(self, out, ldj_mol):
        """``[num_mols]``: element m is what ``__call__`` returns for molecule m
        alone as a batch of one with ``ldj_mol[m]`` (e.g. from
        ``LFIntegrator.forward(per_molecule=True)``) -- logZ for its own atom
        count and its own two log(2 pi) terms of log_gaussian.  The batch
        scalar counts those two terms once for the whole batch, so

            per_molecule(out, ldj_mol).mean() - self(out, ldj_mol.sum())
                = (M - 1) / M * log(2 pi).

        Inference only (enflow_alchemical_nll_mol_f32 over the per-molecule
        energy rows)."""
        if torch.is_grad_enabled() and isinstance(ldj_mol, torch.Tensor) and ldj_mol.requires_grad:
            raise NotImplementedError("Alchemical_NLL.per_molecule is inference-only (the HIP backward takes the "
                                      "batch scalar): call it under torch.no_grad(), or "
                                      "Alchemical_NLL.per_molecule_grad")
        nll_mol, ptr, M, dev = self._nll_mol(out, "per_molecule")
        ldj_t = torch.as_tensor(ldj_mol, device=dev).detach().to(torch.float32).reshape(-1).contiguous()
        if ldj_t.numel() != M:
            raise ValueError(f"ldj_mol has {ldj_t.numel()} elements, the batch {M} molecules")
        res = torch.empty(max(M, 1), dtype=torch.float32, device=dev)
        L = _lib.lib(out.h.shape[1])
        _lib.check(L.enflow_alchemical_nll_mol_f32(M, _lib.ptr(ptr), _lib.ptr(nll_mol), _lib.ptr(ldj_t),
                                                   float(self.kBT), float(self.z_lj), _lib.ptr(res),
                                                   _lib.stream_ptr(dev)), "enflow_alchemical_nll_mol_f32")
        return res[:M].to(out.h.dtype)

    def _mol_grad(self, out, ldj_mol):
        """potential (ldj_mol None) / per_molecule with a grad_fn (_MolEnergyFunction)."""
        from ._train import _MolEnergyFunction
        dev = out.pos.device
        ptr, max_n = batch_meta(out, dev)
        f = lambda t: t.to(device=dev, dtype=torch.float32)  # noqa: E731
        meta = {"mol_ptr": ptr, "max_n": max_n, "nf": out.h.shape[1]}
        if ldj_mol is None:     # the energy depends on pos alone
            return _MolEnergyFunction.apply(self, meta, f(out.h.detach()), f(out.g.detach()), f(out.pos),
                                            f(out.vel.detach()), None)
        return _MolEnergyFunction.apply(self, meta, f(out.h), f(out.g), f(out.pos), f(out.vel),
                                        ldj_mol.to(device=dev, dtype=torch.float32).reshape(-1))

    def potential_grad(self, out):
        """``potential(out)`` (the same values, bitwise) that is differentiable
        w.r.t. ``out.pos`` -- the energy depends on nothing else -- with a
        ``[num_mols]`` upstream gradient: each molecule's weight reaches its own
        atoms' forces (enflow_alchemical_nll_mol_backward_f32; once
        differentiable).  With autograd off, or ``out.pos`` not requiring a
        gradient, it is ``potential``."""
        _lib.require_gpu(out.pos)
        if not (torch.is_grad_enabled() and out.pos.requires_grad):
            with torch.no_grad():
                return self.potential(out)
        return self._mol_grad(out, None).to(out.h.dtype)

    def per_molecule_grad(self, out, ldj_mol):
        """``per_molecule(out, ldj_mol)`` (the same values, bitwise) that is
        differentiable w.r.t. ``out.h / g / pos / vel`` and ``ldj_mol`` (e.g.
        ``rev_ldj`` of ``LFIntegrator.reverse_grad``) with a ``[num_mols]``
        upstream gradient (enflow_alchemical_nll_mol_backward_f32; once
        differentiable).  With autograd off, or nothing requiring a gradient,
        it is ``per_molecule``."""
        _lib.require_gpu(out.pos)
        ldj_t = torch.as_tensor(ldj_mol)
        M = batch_meta(out, out.pos.device)[0].numel() - 1
        if ldj_t.numel() != M:
            raise ValueError(f"ldj_mol has {ldj_t.numel()} elements, the batch {M} molecules")
        if not (torch.is_grad_enabled() and any(t.requires_grad for t in (out.h, out.g, out.pos, out.vel, ldj_t))):
            with torch.no_grad():
                return self.per_molecule(out, ldj_t)
        return self._mol_grad(out, ldj_t).to(out.h.dtype)

    def _differentiable(self, out, ldj):
        """Same value, with a grad_fn whose backward is enflow_alchemical_nll_backward_f32."""
        from ._train import _NLLFunction
        dev = out.pos.device
        ptr, max_n = batch_meta(out, dev)
        f = lambda t: t.to(device=dev, dtype=torch.float32)  # noqa: E731
        ldj_t = torch.as_tensor(ldj, device=dev)
        loss = _NLLFunction.apply(self, {"mol_ptr": ptr, "max_n": max_n}, f(out.h), f(out.g), f(out.pos),
                                  f(out.vel), ldj_t.to(torch.float32).reshape(()))
        return loss.to(out.h.dtype)

"""``DftHamiltonianBlock`` and ``mul_`` -- host mirror of src/terms/Hamiltonian.jl:22-57,137-192.

Kinetic multiplier, sphere tables and projectors live in the k-block handle of the device library; the
block OWNS its summed local potential (operators.jl:213-222) like the reference's block owns its operators.
The device handle holds one padded copy of a potential at a time: every entry point that applies H
(``mul_``, ``lobpcg_hyper``) calls ``bind()``, which re-uploads this block's potential when another block
of the same k-point (an older / newer Hamiltonian that is still alive) was the last one bound.
"""
from __future__ import annotations

import torch

from . import _lib


class DftHamiltonianBlock:
    def __init__(self, basis, kpoint, potential, bind: bool = True):
        basis._require_gpu()
        self.basis, self.kpoint = basis, kpoint
        self.potential = potential.to(torch.float64).contiguous() if potential is not None else None
        # the exchange term of this block (exchange.ExchangeOperator; models with ExactExchange only): like the potential,
        # the device handle holds one at a time -- in its projector slot -- and bind() puts this block's back
        self.exchange = None
        # the Hubbard term of this block (hubbard.HubbardOperator; models with a Hubbard term and occupation matrices only):
        # rotated orbitals behind P in the same projector slot
        self.hubbard = None
        # the cube v_tau = de/dtau of a meta-GGA (None otherwise): with it bound the handle adds -1/2 div(v_tau grad psi)
        self.tau_potential = None
        if bind:
            self.bind(force=True)

    @staticmethod
    def for_all_kpoints(basis, potential, exchange=None, hubbard=None, tau_potential=None):
        """The blocks of every local k-point for ONE summed potential (Hamiltonian.jl:36-57), bound with a single library
        call (``dftk_mi_kblocks_set_potential``) instead of one host round trip per k-point.  ``exchange`` (models with
        ExactExchange): {k-block index: ExchangeOperator}, attached BEFORE the blocks are bound, so that the projector slot is
        set once per Hamiltonian.  ``hubbard`` (models with a Hubbard term): {k-block index: HubbardOperator}, likewise.
        ``tau_potential`` (meta-GGA): the cube de/dtau of all blocks, bound with a single library call as well
        (``dftk_mi_kblocks_set_tau_potential``: the blocks of a basis handle share ONE padded copy, like the potential); a block
        that is bound again later, by its own ``bind()``, gets a copy of its own."""
        import ctypes as C

        def attach(blocks):
            if tau_potential is not None:
                vt = tau_potential.to(torch.float64).contiguous()
                for b_ in blocks:
                    b_.tau_potential = vt
            if hubbard is not None:
                for ik, b_ in enumerate(blocks):
                    b_.hubbard = hubbard.get(ik)
            if exchange is not None:
                for ik, b_ in enumerate(blocks):
                    b_.exchange = exchange.get(ik)
                    b_.kpoint._exx_owner = None
            return blocks
        if potential is not None and potential.dim() == 4:
            # collinear spin: potential[s] belongs to the k-blocks of spin s + 1 (xc.jl:163-175: Vxc[:, :, :, kpt.spin])
            pots = [potential[s_].to(torch.float64).contiguous() for s_ in range(potential.shape[0])]
            blocks = attach([DftHamiltonianBlock(basis, kpt, pots[kpt.spin - 1], bind=False) for kpt in basis.kpoints])
            basis.pre_call()
            for s_, pot_s in enumerate(pots):
                mine = [b_ for b_ in blocks if b_.kpoint.spin == s_ + 1]
                kbs = (C.c_void_p * len(mine))(*[b_.kpoint.handle.value for b_ in mine])
                _lib.check(basis.lib.dftk_mi_kblocks_set_potential(len(mine), kbs, pot_s.data_ptr()))
            for b_ in blocks:
                b_.kpoint._pot_owner = b_
                b_.bind()                      # (the potential is in place: the exchange operator, if any)
            return blocks
        pot = potential.to(torch.float64).contiguous() if potential is not None else None
        blocks = attach([DftHamiltonianBlock(basis, kpt, pot, bind=False) for kpt in basis.kpoints])
        if pot is None or len(blocks) < 2:
            for b_ in blocks:
                b_.bind(force=True)
            return blocks
        n = len(blocks)
        kbs = (C.c_void_p * n)(*[b_.kpoint.handle.value for b_ in blocks])
        basis.pre_call()
        _lib.check(basis.lib.dftk_mi_kblocks_set_potential(n, kbs, pot.data_ptr()))
        if tau_potential is not None:
            vt = blocks[0].tau_potential
            for b_ in blocks:
                b_._set_frame()
            _lib.check(basis.lib.dftk_mi_kblocks_set_tau_potential(n, kbs, vt.data_ptr()))
            for b_ in blocks:
                b_.kpoint._tau_bound = vt
        for b_ in blocks:
            b_.kpoint._pot_owner = b_
            b_.bind()
        return blocks

    def _set_frame(self):
        """Tell the device handle its k-point and the reciprocal lattice (once): what turns the integer G of a row into
        (G + k) in cartesian coordinates for the div-A-grad term."""
        kpt = self.kpoint
        if not getattr(kpt, "_frame_set", False):
            import numpy as np
            Bh = np.asfortranarray(self.basis.model.recip_lattice, dtype=np.float64)
            kc = np.ascontiguousarray(kpt.coordinate, dtype=np.float64)
            _lib.check(self.basis.lib.dftk_mi_kblock_set_kpoint(kpt.handle, Bh.ctypes.data, kc.ctypes.data))
            kpt._frame_set = True

    def bind(self, force: bool = False):
        """Make the device handle of the k-point apply THIS block's potential."""
        kpt = self.kpoint
        if force or kpt._pot_owner is not self:
            if self.potential is not None:
                self.basis.pre_call()
                _lib.check(self.basis.lib.dftk_mi_kblock_set_potential(kpt.handle, self.potential.data_ptr()))
            else:
                _lib.check(self.basis.lib.dftk_mi_kblock_set_potential(kpt.handle, None))
            kpt._pot_owner = self
        if self._has_exchange_term() and (force or getattr(kpt, "_exx_owner", None) is not self):
            from .exchange import bind_projectors
            xi = self.exchange.xi if self.exchange is not None else None
            bind_projectors(self.basis, self.basis.kpoints.index(kpt), xi)
            kpt._exx_owner = self
        # (likewise without a meta-GGA: the blocks carry None and nothing is bound)
        if getattr(kpt, "_tau_bound", None) is not self.tau_potential:
            lib = self.basis.lib
            if self.tau_potential is not None:
                self._set_frame()
                self.basis.pre_call()
                _lib.check(lib.dftk_mi_kblock_set_tau_potential(kpt.handle, self.tau_potential.data_ptr()))
            else:
                _lib.check(lib.dftk_mi_kblock_set_tau_potential(kpt.handle, None))
            kpt._tau_bound = self.tau_potential
        # (a model without Hubbard term never leaves the first test: its blocks carry None and the slot holds None)
        if getattr(kpt, "_hubbard_bound", None) is not self.hubbard:
            from .hubbard import bind_projector_rows
            bind_projector_rows(self.basis, self.basis.kpoints.index(kpt), self.hubbard)
            kpt._hubbard_bound = self.hubbard

    def _has_exchange_term(self):
        return getattr(self.basis.terms, "exx_kernel", None) is not None

    def set_exchange(self, op):
        """Attach the exchange operator this Hamiltonian was built with (None: no orbitals yet, the term is absent) and
        bind it."""
        self.exchange = op
        self.kpoint._exx_owner = None
        self.bind()

    @property
    def n_G(self):
        return self.kpoint.n_G

    @property
    def n_loc(self):
        """Rows of an orbital block on this rank (== n_G unless the basis shards plane waves)."""
        return self.kpoint.n_loc

    def size(self):
        return (self.kpoint.n_G, self.kpoint.n_G)

    def mul_(self, Hpsi: torch.Tensor, psi: torch.Tensor, which: int = 7) -> torch.Tensor:
        """``mul!(Hpsi, H, psi)``: psi, Hpsi are (n_bands, ld >= n_G) complex128 CUDA tensors whose rows
        are bands (column-major n_G x n_bands)."""
        if not (psi.is_cuda and Hpsi.is_cuda and psi.dtype == torch.complex128 and Hpsi.dtype == torch.complex128):
            raise TypeError("mul_: complex128 CUDA tensors required (the hot path has no CPU fallback)")
        if psi.dim() != 2 or psi.stride(1) != 1 or Hpsi.stride(1) != 1:
            raise ValueError("mul_: band-major contiguous blocks required")
        nb = psi.shape[0]
        if psi.shape[1] != self.n_loc or Hpsi.shape != psi.shape:
            raise ValueError(f"mul_: blocks must be (n_bands, {self.n_loc})")
        self.bind()
        self.basis.pre_call()
        _lib.check(self.basis.lib.dftk_mi_apply_H_parts(self.kpoint.handle, which, nb, psi.data_ptr(), psi.stride(0),
                                                        Hpsi.data_ptr(), Hpsi.stride(0)))
        if which & 4 and self.exchange is not None and self.exchange.psi_occ is not None:
            # the uncompressed exchange operator (VanillaExx) is no projector term: its own pass, added to H psi
            from .exchange import apply_exchange
            apply_exchange(self.basis, self.basis.kpoints.index(self.kpoint), self.exchange.psi_occ, self.exchange.occ, psi,
                           out=Hpsi, accumulate=True)
        self.basis.post_call(self.kpoint.lane)
        return Hpsi

    def __matmul__(self, psi):
        return self.mul_(torch.empty_like(psi), psi)


def mul_(Hpsi, H: DftHamiltonianBlock, psi):
    """Free-function spelling of ``mul!(Hpsi, H, psi)``."""
    return H.mul_(Hpsi, psi)

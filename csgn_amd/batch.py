"""Torch-backed plumbing over the C ABI: device buffers, streams, batch calls.

PyTorch is used here ONLY for HBM allocation (`torch.empty(..., device="cuda")`), the current
HIP stream and `torch.distributed`; every arithmetic result comes from libcsgn_hip.so through
`csgn_amd.capi`.  Term words are uint64 on the wire; torch holds them as int64 (same bits).

All methods enqueue on torch's current stream, so `torch.cuda.Event` brackets them correctly.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import capi
from .capi import check


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


class HipPath:
    """One GPU's view of the hot path.  Construct one per process / device."""

    def __init__(self, device: int = 0):
        self.lib = capi.load_library()
        if not torch.cuda.is_available():
            raise capi.CsgnError(capi.CSGN_ERR_NO_DEVICE,
                                 "torch sees no GPU; csgn_amd has no CPU fallback")
        torch.cuda.set_device(device)
        check(self.lib.csgn_init(device))
        self.device = torch.device("cuda", device)

    def close(self) -> None:
        """Destroys the calling thread's csgn_mul_plan handle (its device block goes back to the driver).  Handles of
        other threads are destroyed when those threads call close(), or with the process."""
        plans = getattr(self, "_plans", None)
        handle = getattr(plans, "handle", None) if plans is not None else None
        if handle is not None:
            self.lib.csgn_mul_plan_destroy(handle)
            plans.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing -------------------------------------------------------------------
    @property
    def stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def empty_words(self, n_words: int) -> torch.Tensor:
        return torch.empty(int(n_words), dtype=torch.int64, device=self.device)

    def upload(self, a: np.ndarray) -> torch.Tensor:
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            return torch.from_numpy(a.view(np.int64)).to(self.device)
        if a.dtype == np.uint32:
            return torch.from_numpy(a.view(np.int32)).to(self.device)
        return torch.from_numpy(a).to(self.device)

    @staticmethod
    def download(t: torch.Tensor) -> np.ndarray:
        a = t.detach().cpu().numpy()
        if a.dtype == np.int64:
            return a.view(np.uint64)
        if a.dtype == np.int32:
            return a.view(np.uint32)
        return a

    def default_len(self, n_bits: int) -> int:
        return int(self.lib.csgn_default_len(n_bits))

    def key_mask(self, n_bits: int, key) -> np.ndarray:
        key = np.ascontiguousarray(np.asarray(key, dtype=np.uint64))
        mask = np.zeros(self.default_len(n_bits), dtype=np.uint64)
        check(self.lib.csgn_key_mask(n_bits, key.ctypes.data, key.size, mask.ctypes.data))
        return mask

    # -- multiply -------------------------------------------------------------------
    def mul_uniform(self, n_bits: int, batch: int, t1: int, t2: int, left: torch.Tensor,
                    right: torch.Tensor, out: Optional[torch.Tensor] = None,
                    out_slots: int = 0) -> torch.Tensor:
        dl = self.default_len(n_bits)
        assert left.numel() >= batch * t1 * dl and right.numel() >= batch * t2 * dl
        slots = batch if out_slots == 0 else min(out_slots, batch)
        if out is None:
            out = self.empty_words(slots * t1 * t2 * dl)
        assert out.numel() >= slots * t1 * t2 * dl
        check(self.lib.csgn_mul_uniform(n_bits, batch, t1, t2, _ptr(left), _ptr(right), _ptr(out),
                                        out_slots, self.stream))
        return out

    def mul_ragged(self, n_bits: int, left: torch.Tensor, off_left: torch.Tensor,
                   right: torch.Tensor, off_right: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Plan (csgn_mul_plan_ragged, synchronises) + multiply by that plan (csgn_mul_planned)."""
        batch = off_left.numel() - 1
        dl = self.default_len(n_bits)
        off_out = self.empty_words(batch + 1)
        plan = (C.c_uint64 * 4)()
        # one plan object per path AND host thread (a csgn_mul_plan is used by one thread at a time); its
        # device block is grow-only, so the plan costs no allocation after the first call
        import threading
        if getattr(self, "_plans", None) is None:
            self._plans = threading.local()
        if getattr(self._plans, "handle", None) is None:
            self._plans.handle = self.mul_plan()
        handle = self._plans.handle
        check(self.lib.csgn_mul_plan_ragged(handle, batch, _ptr(off_left), _ptr(off_right), _ptr(off_out),
                                            C.byref(plan), self.stream))
        total = int(plan[0])
        out = self.empty_words(max(total * dl, 1))
        check(self.lib.csgn_mul_planned(handle, n_bits, _ptr(left), _ptr(right), _ptr(out), self.stream))
        return out[: total * dl], off_out

    def mul_plan(self) -> C.c_void_p:
        """A csgn_mul_plan object (destroy with lib.csgn_mul_plan_destroy)."""
        handle = C.c_void_p()
        check(self.lib.csgn_mul_plan_create(C.byref(handle)))
        return handle

    def mul_ragged_async(self, n_bits: int, left: torch.Tensor, off_left: torch.Tensor, right: torch.Tensor,
                         off_right: torch.Tensor, capacity_terms: int, out: Optional[torch.Tensor] = None,
                         off_out: Optional[torch.Tensor] = None, plan: Optional[torch.Tensor] = None):
        """csgn_mul_ragged_async: nothing is read back.  Returns (out, off_out, d_plan); mul_ragged_async_result(d_plan)
        fetches the plan numbers and the does-not-fit flag later."""
        batch = off_left.numel() - 1
        dl = self.default_len(n_bits)
        if off_out is None:
            off_out = self.empty_words(batch + 1)
        if out is None:
            out = self.empty_words(max(capacity_terms * dl, 1))
        if plan is None:
            plan = self.empty_words(int(self.lib.csgn_mul_ragged_async_plan_words(batch)))
        check(self.lib.csgn_mul_ragged_async(n_bits, batch, _ptr(left), _ptr(off_left), _ptr(right), _ptr(off_right),
                                             _ptr(out), _ptr(off_out), capacity_terms, _ptr(plan), self.stream))
        return out, off_out, plan

    def mul_ragged_async_result(self, plan: torch.Tensor):
        res = (C.c_uint64 * 5)()
        check(self.lib.csgn_mul_ragged_async_result(_ptr(plan), C.byref(res), self.stream))
        return [int(x) for x in res]

    # -- add ------------------------------------------------------------------------
    def add_uniform(self, n_bits: int, batch: int, t1: int, t2: int, left: torch.Tensor,
                    right: torch.Tensor) -> torch.Tensor:
        dl = self.default_len(n_bits)
        out = self.empty_words(max(batch * (t1 + t2) * dl, 1))
        check(self.lib.csgn_add_uniform(n_bits, batch, t1, t2, _ptr(left), _ptr(right), _ptr(out),
                                        self.stream))
        return out[: batch * (t1 + t2) * dl]

    # -- gates ----------------------------------------------------------------------
    def gate_uniform(self, n_bits: int, gate: int, batch: int, a: torch.Tensor, t_a: int,
                     b: Optional[torch.Tensor] = None, t_b: int = 0, sel: Optional[torch.Tensor] = None,
                     t_sel: int = 0, plain: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """csgn_gate_uniform: one of capi.CSGN_GATE_* over a uniform batch (plain: uint8 tensor, one bit per element).
        A fresh tensor unless `out` is given."""
        dl = self.default_len(n_bits)
        terms = int(self.lib.csgn_gate_terms(gate, t_sel, t_a, t_b))
        assert terms, "bad gate or shape"
        if out is None:
            out = self.empty_words(max(batch * terms * dl, 1))
        assert out.numel() >= batch * terms * dl
        check(self.lib.csgn_gate_uniform(n_bits, gate, batch, t_sel, t_a, t_b, _ptr(sel), _ptr(a), _ptr(b),
                                         _ptr(plain), _ptr(out), self.stream))
        return out[: batch * terms * dl]

    def const_fill(self, n_bits: int, batch: int, plain: Optional[torch.Tensor] = None, bit: int = 1) -> torch.Tensor:
        """csgn_const_fill: `batch` 1-term constants, ONE where plain & 1 (or `bit` when plain is None), else ZERO."""
        dl = self.default_len(n_bits)
        out = self.empty_words(max(batch * dl, 1))
        check(self.lib.csgn_const_fill(n_bits, batch, _ptr(plain), int(bit), _ptr(out), self.stream))
        return out[: batch * dl]

    # -- bit-sliced integers ----------------------------------------------------------
    def uint_step(self, n_bits: int, step: int, batch: int, a: torch.Tensor, t_a: int, b: torch.Tensor, t_b: int,
                  x: Optional[torch.Tensor] = None, t_x: int = 0, carry: bool = True, outs=None):
        """csgn_uint_step: one of capi.CSGN_UINT_* over a uniform batch.  Returns the output tensor, or (sum, carry) for
        the ADD steps when `carry` (carry=False passes a null carry pointer: the carry is not computed).  Fresh tensors
        unless `outs` (one tensor, two with a carry) is given."""
        dl = self.default_len(n_bits)
        has_carry = carry and step in (capi.CSGN_UINT_ADD_HALF, capi.CSGN_UINT_ADD_FULL)
        terms0 = int(self.lib.csgn_uint_step_terms(step, 0, t_x, t_a, t_b))
        terms1 = int(self.lib.csgn_uint_step_terms(step, 1, t_x, t_a, t_b)) if has_carry else 0
        assert terms0 and (terms1 or not has_carry), "bad step or shape"
        if outs is None:
            outs = [self.empty_words(max(batch * terms0 * dl, 1))]
            if has_carry:
                outs.append(self.empty_words(max(batch * terms1 * dl, 1)))
        assert len(outs) == (2 if has_carry else 1)
        out0, out1 = outs[0], (outs[1] if has_carry else None)
        assert out0.numel() >= batch * terms0 * dl and (out1 is None or out1.numel() >= batch * terms1 * dl)
        check(self.lib.csgn_uint_step(n_bits, step, batch, _ptr(x), t_x, _ptr(a), t_a, _ptr(b), t_b, _ptr(out0),
                                      _ptr(out1), self.stream))
        if has_carry:
            return out0[: batch * terms0 * dl], out1[: batch * terms1 * dl]
        return out0[: batch * terms0 * dl]

    def uint_plain(self, n_bits: int, cmp: int, batch: int, planes, terms, k: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """csgn_uint_plain: one of capi.CSGN_UINT_PLAIN_* of the w-bit integer `planes` (bit 0 first; plane j a uniform
        batch of terms[j] terms per element) against the public constant k.  Returns the output tensor (a fresh one
        unless `out` is given)."""
        w = len(planes)
        assert w == len(terms)
        h_terms = (C.c_uint64 * max(w, 1))(*[int(t) for t in terms])
        h_planes = (C.c_void_p * max(w, 1))(*[_ptr(p) for p in planes])
        total = int(self.lib.csgn_uint_plain_terms(cmp, w, k, h_terms))
        assert total, "bad comparison or shape"
        dl = self.default_len(n_bits)
        if out is None:
            out = self.empty_words(max(batch * total * dl, 1))
        assert out.numel() >= batch * total * dl
        check(self.lib.csgn_uint_plain(n_bits, cmp, batch, w, k, h_planes, h_terms, _ptr(out), self.stream))
        return out[: batch * total * dl]

    def uint_addk_terms(self, terms, k: int):
        """csgn_uint_addk_terms: the terms per element of every plane of a + k and, last, of the carry-out; None for an
        invalid shape."""
        w = len(terms)
        h_terms = (C.c_uint64 * max(w, 1))(*[int(t) for t in terms])
        out = (C.c_uint64 * (w + 1))()
        return list(out) if self.lib.csgn_uint_addk_terms(w, k, h_terms, out) else None

    def uint_addk(self, n_bits: int, batch: int, planes, terms, k: int, negate: bool = False, carry: bool = False,
                  outs=None, carry_out: Optional[torch.Tensor] = None):
        """csgn_uint_addk: the w-bit integer `planes` (bit 0 first; plane j a uniform batch of terms[j] terms per
        element) plus the public constant k, ONE appended to every plane when `negate`.  Returns (output tensors,
        carry-out tensor or None); fresh tensors unless `outs` / `carry_out` are given."""
        w = len(planes)
        assert w == len(terms)
        T = self.uint_addk_terms(terms, k)
        assert T, "bad width, constant or shape"
        dl = self.default_len(n_bits)
        sizes = [batch * (t + (1 if negate else 0)) * dl for t in T[:w]]
        if outs is None:
            outs = [self.empty_words(max(s, 1)) for s in sizes]
        if carry and carry_out is None:
            carry_out = self.empty_words(max(batch * T[w] * dl, 1))
        h_terms = (C.c_uint64 * w)(*[int(t) for t in terms])
        h_planes = (C.c_void_p * w)(*[_ptr(p) for p in planes])
        h_outs = (C.c_void_p * w)(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_addk(n_bits, batch, w, k, 1 if negate else 0, h_planes, h_terms, h_outs,
                                      _ptr(carry_out) if carry else None, self.stream))
        return [o[:s] for o, s in zip(outs, sizes)], (carry_out[: batch * T[w] * dl] if carry else None)

    def uint_lut_create(self, table, in_width: int, out_width: int, terms) -> int:
        """csgn_uint_lut_create: the public table (2^in_width entries < 2^out_width) compiled for planes of terms[i] terms
        per element.  Returns the handle; release it with self.lib.csgn_uint_lut_destroy."""
        h_table = (C.c_uint64 * len(table))(*[int(v) for v in table])
        h_terms = (C.c_uint64 * max(len(terms), 1))(*[int(t) for t in terms])
        handle = C.c_void_p()
        check(self.lib.csgn_uint_lut_create(in_width, out_width, h_table, h_terms, C.byref(handle)))
        return handle.value

    def uint_lut_apply(self, handle: int, n_bits: int, batch: int, planes, out_terms, outs=None):
        """csgn_uint_lut_apply of a compiled table: planes bit 0 first, out_terms[j] = T_j.  Returns the output tensors
        (fresh ones unless `outs` is given)."""
        dl = self.default_len(n_bits)
        if outs is None:
            outs = [self.empty_words(max(batch * int(t) * dl, 1)) for t in out_terms]
        h_planes = (C.c_void_p * max(len(planes), 1))(*[_ptr(p) for p in planes])
        h_out = (C.c_void_p * len(outs))(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_lut_apply(handle, n_bits, batch, h_planes, h_out, self.stream))
        return [o[: batch * int(t) * dl] for o, t in zip(outs, out_terms)]

    def uint_lut(self, n_bits: int, batch: int, planes, terms, table, out_width: int, outs=None):
        """The public lookup table `table` applied to the w-bit integer `planes` (bit 0 first; plane i a uniform batch of
        terms[i] terms per element): one tensor per output bit, T_j terms per element (csgn_uint_lut_terms); fresh ones
        unless `outs` is given."""
        w = len(planes)
        assert w == len(terms) and len(table) == 1 << w
        h_table = (C.c_uint64 * len(table))(*[int(v) for v in table])
        h_terms = (C.c_uint64 * w)(*[int(t) for t in terms])
        out_terms = (C.c_uint64 * out_width)()
        check(self.lib.csgn_uint_lut_terms(w, out_width, h_table, h_terms, out_terms))
        handle = self.uint_lut_create(table, w, out_width, terms)
        try:
            outs = self.uint_lut_apply(handle, n_bits, batch, planes, list(out_terms), outs)
            torch.cuda.current_stream(self.device).synchronize()
        finally:
            self.lib.csgn_uint_lut_destroy(handle)
        return outs

    def gather_plan(self, count_in: int, count_out: int, index: Optional[torch.Tensor] = None,
                    src_off: Optional[torch.Tensor] = None, out_off: Optional[torch.Tensor] = None):
        """csgn_gather_plan (synchronous).  Returns (rc, total output terms, bad indices, out_off): rc is CSGN_OK or
        CSGN_ERR_INVALID when an index is >= count_in (then out_off is not written); it does not raise for that case.
        A ragged source (src_off given) gets fresh output offsets unless `out_off` is given."""
        if src_off is not None and out_off is None:
            out_off = self.empty_words(count_out + 1)
        res = (C.c_uint64 * 2)()
        rc = self.lib.csgn_gather_plan(count_in, _ptr(src_off), count_out, _ptr(index), _ptr(out_off), res, self.stream)
        if rc not in (capi.CSGN_OK, capi.CSGN_ERR_INVALID) or (rc != capi.CSGN_OK and res[1] == 0):
            check(rc)
        return rc, int(res[0]), int(res[1]), out_off

    def gather(self, n_bits: int, count_in: int, src: torch.Tensor, t_src: int, count_out: int,
               index: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """csgn_gather of a uniform source (t_src terms per element): element e of the result is source element
        index[e], or e mod count_in without an index list (tile / broadcast).  The indices must be valid (a plan's)."""
        dl = self.default_len(n_bits)
        if out is None:
            out = self.empty_words(max(count_out * t_src * dl, 1))
        check(self.lib.csgn_gather(n_bits, count_in, _ptr(src), None, t_src, count_out, _ptr(index), _ptr(out), None, 0,
                                   self.stream))
        return out[: count_out * t_src * dl]

    def gather_ragged(self, n_bits: int, count_in: int, src: torch.Tensor, src_off: torch.Tensor, count_out: int,
                      index: Optional[torch.Tensor] = None, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Plan + gather of a ragged (CSR) source; returns (words, output offsets).  Raises on a bad index.  `out`: a
        function of the planned word count that gives the tensor to write (default: a fresh one)."""
        rc, total, bad, out_off = self.gather_plan(count_in, count_out, index, src_off)
        check(rc)
        dl = self.default_len(n_bits)
        out = self.empty_words(max(total * dl, 1)) if out is None else out(total * dl)
        check(self.lib.csgn_gather(n_bits, count_in, _ptr(src), _ptr(src_off), 0, count_out, _ptr(index), _ptr(out),
                                   _ptr(out_off), total, self.stream))
        return out[: total * dl], out_off

    def gather_planes(self, n_bits: int, planes, terms, count_in: int, count_out: int,
                      index: Optional[torch.Tensor] = None, outs=None):
        """csgn_gather_planes: every uniform plane (plane j: terms[j] terms per element) gathered by one index list (or
        the tile form) in one launch.  Returns the output tensors."""
        dl = self.default_len(n_bits)
        if outs is None:
            outs = [self.empty_words(max(count_out * int(t) * dl, 1)) for t in terms]
        n = len(planes)
        h_src = (C.c_void_p * n)(*[_ptr(p) for p in planes])
        h_dst = (C.c_void_p * n)(*[_ptr(o) for o in outs])
        h_terms = (C.c_uint64 * n)(*[int(t) for t in terms])
        check(self.lib.csgn_gather_planes(n_bits, n, h_src, h_terms, count_in, count_out, _ptr(index), h_dst,
                                          self.stream))
        return [o[: count_out * int(t) * dl] for o, t in zip(outs, terms)]

    def uint_read(self, n_bits: int, batch: int, index, index_terms, rows: int, table, table_terms, outs=None):
        """csgn_uint_read: the encrypted table `table` (planes of `rows` elements, plane j uniform with table_terms[j]
        terms) read at the encrypted index `index` (bit 0 first; plane k a uniform batch of index_terms[k] terms).  One
        tensor per table plane, table_terms[j] * E terms per element (E = csgn_uint_read_terms); fresh ones unless
        `outs` is given."""
        v, w = len(index), len(table)
        assert v == len(index_terms) and w == len(table_terms)
        h_s = (C.c_uint64 * max(v, 1))(*[int(t) for t in index_terms])
        h_t = (C.c_uint64 * max(w, 1))(*[int(t) for t in table_terms])
        E = int(self.lib.csgn_uint_read_terms(v, h_s, rows))
        assert E, "bad index width, rows or term count"
        dl = self.default_len(n_bits)
        if outs is None:
            outs = [self.empty_words(max(batch * int(t) * E * dl, 1)) for t in table_terms]
        h_x = (C.c_void_p * max(v, 1))(*[_ptr(p) for p in index])
        h_d = (C.c_void_p * max(w, 1))(*[_ptr(p) for p in table])
        h_out = (C.c_void_p * max(w, 1))(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_read(n_bits, batch, v, h_x, h_s, rows, w, h_d, h_t, h_out, self.stream))
        return [o[: batch * int(t) * E * dl] for o, t in zip(outs, table_terms)]

    def uint_find(self, n_bits: int, batch: int, query, query_terms, rows: int, keys, key_terms, values, value_terms,
                  outs=None, member=False):
        """csgn_uint_find: the encrypted table of `rows` rows -- key planes `keys` (plane k uniform with key_terms[k]
        terms) and value planes `values` (plane j uniform with value_terms[j] terms) -- looked up by the encrypted
        `query` (plane k a uniform batch of query_terms[k] terms).  Returns (output tensors, member tensor or None): one
        tensor per value plane, rows * P * value_terms[j] terms per element (P = csgn_uint_find_terms), fresh ones
        unless `outs` is given; `member`: True for a fresh tensor of rows * P terms per element, or the tensor to
        write."""
        v, w = len(query), len(values)
        assert v == len(query_terms) == len(keys) == len(key_terms) and w == len(value_terms)
        h_u = (C.c_uint64 * max(v, 1))(*[int(t) for t in key_terms])
        h_s = (C.c_uint64 * max(v, 1))(*[int(t) for t in query_terms])
        h_t = (C.c_uint64 * max(w, 1))(*[int(t) for t in value_terms])
        P = int(self.lib.csgn_uint_find_terms(v, h_u, h_s))
        assert P, "bad key width or term count"
        dl = self.default_len(n_bits)
        E = rows * P
        if outs is None:
            outs = [self.empty_words(max(batch * int(t) * E * dl, 1)) for t in value_terms]
        if member is True:
            member = self.empty_words(max(batch * E * dl, 1))
        elif member is False:
            member = None
        h_x = (C.c_void_p * max(v, 1))(*[_ptr(p) for p in query])
        h_y = (C.c_void_p * max(v, 1))(*[_ptr(p) for p in keys])
        h_d = (C.c_void_p * max(w, 1))(*[_ptr(p) for p in values])
        h_out = (C.c_void_p * max(w, 1))(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_find(n_bits, batch, v, h_x, h_s, rows, h_y, h_u, w, h_d, h_t, h_out, _ptr(member),
                                      self.stream))
        return ([o[: batch * int(t) * E * dl] for o, t in zip(outs, value_terms)],
                None if member is None else member[: batch * E * dl])

    def uint_first(self, n_bits: int, batch: int, group: int, mask, mask_terms, values=(), value_terms=(), outs=None,
                   any=False, labels=None, label_bits=(), label_outs=None):
        """csgn_uint_first: of the `group` rows of every output element the FIRST whose encrypted mask bit is set.
        `mask`: one grouped tensor of batch * group elements (every row of mask_terms[0] terms) or `group` tensors of
        `batch` elements (row r of mask_terms[r] terms); `values`: grouped planes, plane j uniform with value_terms[j]
        terms; `labels`: the rows' public constants, `label_bits` the strictly ascending planes of them to write.
        Returns (output tensors, any tensor or None, label tensors): output j of Q * value_terms[j] terms per element
        (Q = csgn_uint_first_terms(group, mask_terms, group)), any of Q, label plane i of csgn_uint_first_label_terms;
        fresh ones unless `outs` / `label_outs` are given; `any`: True for a fresh tensor, or the tensor to write."""
        g, w, nl = int(group), len(values), len(label_bits)
        assert len(mask) in (1, g) and len(mask_terms) == g and w == len(value_terms)
        h_s = (C.c_uint64 * max(g, 1))(*[int(t) for t in mask_terms])
        h_t = (C.c_uint64 * max(w, 1))(*[int(t) for t in value_terms])
        h_l = (C.c_uint64 * max(g, 1))(*[int(x) for x in (labels if nl else [0] * g)])
        h_b = (C.c_uint64 * max(nl, 1))(*[int(x) for x in label_bits])
        Q = int(self.lib.csgn_uint_first_terms(g, h_s, g))
        T = [int(self.lib.csgn_uint_first_label_terms(g, h_s, h_l, int(x))) for x in label_bits]
        assert (Q or not (w or any is not False)) and all(T), "bad group, term count or label plane"
        dl = self.default_len(n_bits)
        if outs is None:
            outs = [self.empty_words(max(batch * int(t) * Q * dl, 1)) for t in value_terms]
        if label_outs is None:
            label_outs = [self.empty_words(max(batch * x * dl, 1)) for x in T]
        if any is True:
            any = self.empty_words(max(batch * Q * dl, 1))
        elif any is False:
            any = None
        h_m = (C.c_void_p * len(mask))(*[_ptr(p) for p in mask])
        h_d = (C.c_void_p * max(w, 1))(*[_ptr(p) for p in values])
        h_out = (C.c_void_p * max(w, 1))(*[_ptr(o) for o in outs])
        h_lo = (C.c_void_p * max(nl, 1))(*[_ptr(o) for o in label_outs])
        check(self.lib.csgn_uint_first(n_bits, batch, g, h_m, len(mask), h_s, w, h_d, h_t, h_out, _ptr(any), nl, h_l, h_b,
                                       h_lo, self.stream))
        return ([o[: batch * int(t) * Q * dl] for o, t in zip(outs, value_terms)],
                None if any is None else any[: batch * Q * dl],
                [o[: batch * x * dl] for o, x in zip(label_outs, T)])

    def uint_nth(self, n_bits: int, batch: int, group: int, slot: int, mask, mask_terms: int, values=(), value_terms=(),
                 outs=None, valid=False, labels=None, label_bits=(), label_outs=None):
        """csgn_uint_nth: of the `group` rows of every output element the (slot + 1)-th whose encrypted mask bit is set.
        `mask`: one grouped tensor of batch * group elements or `group` tensors of `batch` elements, every row of
        `mask_terms` terms; `values`: grouped planes, plane j uniform with value_terms[j] terms; `labels`: the rows'
        public constants, `label_bits` the strictly ascending planes of them to write.  Returns (output tensors, valid
        tensor or None, label tensors): output j of Q * value_terms[j] terms per element (Q = csgn_uint_nth_terms(group,
        mask_terms, slot, group)), valid of Q, label plane i of csgn_uint_nth_label_terms; fresh ones unless `outs` /
        `label_outs` are given; `valid`: True for a fresh tensor, or the tensor to write."""
        g, s, tm, w, nl = int(group), int(slot), int(mask_terms), len(values), len(label_bits)
        assert len(mask) in (1, g) and w == len(value_terms)
        h_t = (C.c_uint64 * max(w, 1))(*[int(t) for t in value_terms])
        h_l = (C.c_uint64 * max(g, 1))(*[int(x) for x in (labels if nl else [0] * g)])
        h_b = (C.c_uint64 * max(nl, 1))(*[int(x) for x in label_bits])
        Q = int(self.lib.csgn_uint_nth_terms(g, tm, s, g))
        T = [int(self.lib.csgn_uint_nth_label_terms(g, tm, s, h_l, int(x))) for x in label_bits]
        assert Q and all(T), "bad group, slot, term count or label plane"
        dl = self.default_len(n_bits)
        if outs is None:
            outs = [self.empty_words(max(batch * int(t) * Q * dl, 1)) for t in value_terms]
        if label_outs is None:
            label_outs = [self.empty_words(max(batch * x * dl, 1)) for x in T]
        if valid is True:
            valid = self.empty_words(max(batch * Q * dl, 1))
        elif valid is False:
            valid = None
        h_m = (C.c_void_p * len(mask))(*[_ptr(p) for p in mask])
        h_d = (C.c_void_p * max(w, 1))(*[_ptr(p) for p in values])
        h_out = (C.c_void_p * max(w, 1))(*[_ptr(o) for o in outs])
        h_lo = (C.c_void_p * max(nl, 1))(*[_ptr(o) for o in label_outs])
        check(self.lib.csgn_uint_nth(n_bits, batch, g, s, h_m, len(mask), tm, w, h_d, h_t, h_out, _ptr(valid), nl, h_l,
                                     h_b, h_lo, self.stream))
        return ([o[: batch * int(t) * Q * dl] for o, t in zip(outs, value_terms)],
                None if valid is None else valid[: batch * Q * dl],
                [o[: batch * x * dl] for o, x in zip(label_outs, T)])

    def uint_pick(self, n_bits: int, op: int, batch: int, index, index_terms, a, terms: int, rows: int = 0, outs=None):
        """csgn_uint_pick: the encrypted integer `a` (bit 0 first; every plane a uniform batch of `terms` terms)
        shifted or rotated by the encrypted distance `index` (plane k a uniform batch of index_terms[k] terms), op =
        CSGN_UINT_PICK_SHL / SHR / ROTL / ROTR (1..4, rows = 0); or, op = CSGN_UINT_PICK_EACH (5), element e's own array
        of `rows` rows (the elements e * rows .. e * rows + rows - 1 of `a`'s planes) read at its encrypted index.  One
        tensor per plane of `a`, terms * E_j terms per element (E_j = csgn_uint_pick_terms); fresh ones unless `outs` is
        given."""
        v, w = len(index), len(a)
        assert v == len(index_terms)
        h_s = (C.c_uint64 * max(v, 1))(*[int(t) for t in index_terms])
        E = [int(self.lib.csgn_uint_pick_terms(op, v, h_s, w, rows, j)) for j in range(w)]
        assert w and all(E), "bad op, width, rows or term count"
        dl = self.default_len(n_bits)
        if outs is None:
            outs = [self.empty_words(max(batch * int(terms) * e * dl, 1)) for e in E]
        h_x = (C.c_void_p * max(v, 1))(*[_ptr(p) for p in index])
        h_a = (C.c_void_p * max(w, 1))(*[_ptr(p) for p in a])
        h_out = (C.c_void_p * max(w, 1))(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_pick(n_bits, op, batch, v, h_x, h_s, w, rows, h_a, int(terms), h_out, self.stream))
        return [o[: batch * int(terms) * e * dl] for o, e in zip(outs, E)]

    def uint_pick_rows(self, n_bits: int, batch: int, index, index_terms, rows: int, arrays, row_terms, outs=None):
        """csgn_uint_pick_rows: element e's own array of `rows` rows read at its encrypted index `index` (bit 0 first;
        plane k a uniform batch of index_terms[k] terms) where the rows differ in size -- row r of plane j has
        row_terms[j][r] terms in every array, the layout csgn_uint_write leaves.  One uniform tensor per plane, Tout_j
        terms per element (csgn_uint_pick_rows_offsets); fresh ones unless `outs` is given.  The sizes are checked
        (csgn_uint_pick_rows_check) before anything is allocated."""
        v, w = len(index), len(arrays)
        assert v == len(index_terms) and w == len(row_terms) and all(len(t) == rows for t in row_terms)
        h_s = (C.c_uint64 * max(v, 1))(*[int(t) for t in index_terms])
        h_T = (C.c_uint64 * max(w * rows, 1))(*[int(t) for plane in row_terms for t in plane])
        check(self.lib.csgn_uint_pick_rows_check(n_bits, batch, v, h_s, rows, w, h_T))
        src, out = (C.c_uint64 * (rows + 1))(), (C.c_uint64 * (rows + 1))()
        Tout = []
        for j in range(w):
            h_Tj = (C.c_uint64 * rows)(*[int(t) for t in row_terms[j]])
            check(self.lib.csgn_uint_pick_rows_offsets(v, h_s, rows, h_Tj, src, out))
            Tout.append(int(out[rows]))
        dl = self.default_len(n_bits)
        if outs is None:
            outs = [self.empty_words(max(batch * t * dl, 1)) for t in Tout]
        h_x = (C.c_void_p * max(v, 1))(*[_ptr(p) for p in index])
        h_a = (C.c_void_p * max(w, 1))(*[_ptr(p) for p in arrays])
        h_out = (C.c_void_p * max(w, 1))(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_pick_rows(n_bits, batch, v, h_x, h_s, rows, w, h_a, h_T, h_out, self.stream))
        return [o[: batch * t * dl] for o, t in zip(outs, Tout)]

    SCRATCH_STATS = ("blocks", "bytes", "retired", "mallocs", "frees", "tables", "tables_retired", "tables_freed")

    def scratch_stats(self) -> dict:
        """csgn_scratch_stats (host only): the calling thread's scratch blocks and row tables, by SCRATCH_STATS' names."""
        out = (C.c_uint64 * 8)()
        check(self.lib.csgn_scratch_stats(out))
        return dict(zip(self.SCRATCH_STATS, (int(x) for x in out)))

    def uint_write(self, n_bits: int, batch: int, index, index_terms, rows: int, value, value_terms, arrays,
                   array_terms, outs=None):
        """csgn_uint_write: element e's own array of `rows` rows (the elements e * rows .. e * rows + rows - 1 of the
        planes `arrays`, plane j uniform with array_terms[j] terms) written with `value` (plane j a uniform batch of
        value_terms[j] terms) at its encrypted index `index` (bit 0 first; plane k a uniform batch of index_terms[k]
        terms).  One tensor per plane, A_j terms per array (A_j = csgn_uint_write_offset at r = rows), rows ragged
        inside it; fresh ones unless `outs` is given."""
        v, w = len(index), len(value)
        assert v == len(index_terms) and w == len(value_terms) == len(arrays) == len(array_terms)
        h_s = (C.c_uint64 * max(v, 1))(*[int(t) for t in index_terms])
        h_tv = (C.c_uint64 * max(w, 1))(*[int(t) for t in value_terms])
        h_td = (C.c_uint64 * max(w, 1))(*[int(t) for t in array_terms])
        A = [int(self.lib.csgn_uint_write_offset(v, h_s, rows, rows, int(tv), int(td)))
             for tv, td in zip(value_terms, array_terms)]
        assert w and all(A), "bad index width, rows or term count"
        dl = self.default_len(n_bits)
        if outs is None:
            outs = [self.empty_words(max(batch * a * dl, 1)) for a in A]
        h_x = (C.c_void_p * max(v, 1))(*[_ptr(p) for p in index])
        h_v = (C.c_void_p * max(w, 1))(*[_ptr(p) for p in value])
        h_d = (C.c_void_p * max(w, 1))(*[_ptr(p) for p in arrays])
        h_out = (C.c_void_p * max(w, 1))(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_write(n_bits, batch, v, h_x, h_s, rows, w, h_v, h_tv, h_d, h_td, h_out, self.stream))
        return [o[: batch * a * dl] for o, a in zip(outs, A)]

    def uint_lt_select(self, n_bits: int, batch: int, a, a_terms, b, b_terms, xs, x_terms, ys, y_terms, outs=None,
                       less=False):
        """csgn_uint_lt_select: request i is a < b ? xs[i] : ys[i] for the encrypted integers a and b (bit 0 first; plane
        j a uniform batch of a_terms[j] / b_terms[j] terms), xs[i] / ys[i] uniform planes of x_terms[i] / y_terms[i]
        terms.  Returns (output tensors, comparison tensor or None): output i has L * (x_terms[i] + y_terms[i]) +
        y_terms[i] terms per element (L = csgn_uint_lt_terms), fresh ones unless `outs` is given; `less`: True for a
        fresh tensor of L terms per element, or the tensor to write."""
        w, m = len(a), len(xs)
        assert w == len(a_terms) == len(b) == len(b_terms) and m == len(x_terms) == len(ys) == len(y_terms)
        h_ta = (C.c_uint64 * max(w, 1))(*[int(t) for t in a_terms])
        h_tb = (C.c_uint64 * max(w, 1))(*[int(t) for t in b_terms])
        h_tx = (C.c_uint64 * max(m, 1))(*[int(t) for t in x_terms])
        h_ty = (C.c_uint64 * max(m, 1))(*[int(t) for t in y_terms])
        L = int(self.lib.csgn_uint_lt_terms(w, h_ta, h_tb))
        assert L, "bad width or term count"
        dl = self.default_len(n_bits)
        sizes = [batch * (L * (int(tx) + int(ty)) + int(ty)) * dl for tx, ty in zip(x_terms, y_terms)]
        if outs is None:
            outs = [self.empty_words(max(s, 1)) for s in sizes]
        if less is True:
            less = self.empty_words(max(batch * L * dl, 1))
        elif less is False:
            less = None
        h_a = (C.c_void_p * max(w, 1))(*[_ptr(p) for p in a])
        h_b = (C.c_void_p * max(w, 1))(*[_ptr(p) for p in b])
        h_x = (C.c_void_p * max(m, 1))(*[_ptr(p) for p in xs])
        h_y = (C.c_void_p * max(m, 1))(*[_ptr(p) for p in ys])
        h_out = (C.c_void_p * max(m, 1))(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_lt_select(n_bits, batch, w, h_a, h_ta, h_b, h_tb, m, h_x, h_tx, h_y, h_ty, h_out,
                                           _ptr(less), self.stream))
        return [o[:s] for o, s in zip(outs, sizes)], (None if less is None else less[: batch * L * dl])

    def uint_arith(self, n_bits: int, op: int, batch: int, a, a_terms, b, b_terms, outs=None, carry=False):
        """csgn_uint_arith: op = 1 a + b, 2 a - b, 3 a == b, 4 a != b of the encrypted integers a and b (bit 0 first;
        plane j a uniform batch of a_terms[j] / b_terms[j] terms).  Returns (output tensors, carry tensor or None): the
        planes of a sum or difference, or the one result of a comparison, of csgn_uint_arith_terms terms per element,
        fresh ones unless `outs` is given; `carry` (sums and differences): True for a fresh tensor, or the tensor to
        write."""
        w = len(a)
        assert w == len(a_terms) == len(b) == len(b_terms)
        h_ta = (C.c_uint64 * max(w, 1))(*[int(t) for t in a_terms])
        h_tb = (C.c_uint64 * max(w, 1))(*[int(t) for t in b_terms])
        n_out = w if op in (1, 2) else 1
        T = [int(self.lib.csgn_uint_arith_terms(op, w, h_ta, h_tb, o)) for o in range(n_out)]
        assert all(T), "bad operation, width or term count"
        dl = self.default_len(n_bits)
        sizes = [batch * t * dl for t in T]
        if outs is None:
            outs = [self.empty_words(max(s, 1)) for s in sizes]
        csize = batch * int(self.lib.csgn_uint_arith_terms(op, w, h_ta, h_tb, w)) * dl
        if carry is True:
            carry = self.empty_words(max(csize, 1))
        elif carry is False:
            carry = None
        h_a = (C.c_void_p * max(w, 1))(*[_ptr(p) for p in a])
        h_b = (C.c_void_p * max(w, 1))(*[_ptr(p) for p in b])
        h_out = (C.c_void_p * max(n_out, 1))(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_arith(n_bits, op, batch, w, h_a, h_ta, h_b, h_tb, h_out, _ptr(carry), self.stream))
        return [o[:s] for o, s in zip(outs, sizes)], (None if carry is None else carry[:csize])

    def uint_add_where_terms(self, terms, sel_terms: int, k: int):
        """csgn_uint_add_where_terms: the terms per element of every plane of a + (sel ? k : 0) and, last, of the
        carry-out; None for an invalid shape."""
        w = len(terms)
        h_terms = (C.c_uint64 * max(w, 1))(*[int(t) for t in terms])
        out = (C.c_uint64 * (w + 1))()
        return list(out) if self.lib.csgn_uint_add_where_terms(w, k, int(sel_terms), h_terms, out) else None

    def uint_add_where(self, n_bits: int, batch: int, planes, terms, sel, sel_terms: int, k: int, outs=None, carry=False):
        """csgn_uint_add_where: the w-bit integer `planes` (bit 0 first; plane j a uniform batch of terms[j] terms per
        element) plus the public constant k in the elements whose encrypted flag `sel` (a uniform batch of sel_terms
        terms; may be None for k = 0) is set.  Returns (output tensors, carry tensor or None), fresh tensors unless
        `outs` is given; `carry`: True for a fresh tensor, or the tensor to write."""
        w = len(planes)
        assert w == len(terms)
        T = self.uint_add_where_terms(terms, sel_terms, k)
        assert T, "bad width, constant or term count"
        dl = self.default_len(n_bits)
        sizes = [batch * t * dl for t in T[:w]]
        if outs is None:
            outs = [self.empty_words(max(s, 1)) for s in sizes]
        csize = batch * T[w] * dl
        if carry is True:
            carry = self.empty_words(max(csize, 1))
        elif carry is False:
            carry = None
        h_terms = (C.c_uint64 * w)(*[int(t) for t in terms])
        h_planes = (C.c_void_p * w)(*[_ptr(p) for p in planes])
        h_outs = (C.c_void_p * w)(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_add_where(n_bits, batch, w, k, _ptr(sel), int(sel_terms), h_planes, h_terms, h_outs,
                                           _ptr(carry), self.stream))
        return [o[:s] for o, s in zip(outs, sizes)], (None if carry is None else carry[:csize])

    def uint_linear_plan(self, n_bits: int, batch: int, terms, rows, constant: int = 0):
        """csgn_uint_linear_plan: [unit bytes, units per element, G, tiles, workgroups per tile, launches, tile budget,
        plane groups] of a csgn_uint_linear call of this shape under the calling thread's knobs."""
        h_terms = (C.c_uint64 * max(len(terms), 1))(*[int(t) for t in terms])
        h_rows = (C.c_uint64 * max(len(rows), 1))(*[int(r) for r in rows])
        plan = (C.c_uint64 * 8)()
        check(self.lib.csgn_uint_linear_plan(n_bits, batch, len(terms), h_terms, len(rows), h_rows, int(constant), plan))
        return [int(x) for x in plan]

    def uint_linear(self, n_bits: int, batch: int, planes, terms, rows, constant: int = 0, outs=None):
        """csgn_uint_linear: the public matrix `rows` over F2 (rows[j]: the mask of the input planes output plane j
        sums) applied to the encrypted integer `planes` (bit 0 first; plane i a uniform batch of terms[i] terms per
        element), plus ONE in the planes whose bit of `constant` is set.  Returns the output planes, of
        csgn_uint_linear_terms terms per element, fresh ones unless `outs` is given."""
        w, m = len(planes), len(rows)
        assert w == len(terms)
        h_terms = (C.c_uint64 * max(w, 1))(*[int(t) for t in terms])
        T = [int(self.lib.csgn_uint_linear_terms(w, h_terms, int(rows[j]), (int(constant) >> j) & 1)) for j in range(m)]
        assert m and all(T), "bad width, row or term count"
        dl = self.default_len(n_bits)
        sizes = [batch * t * dl for t in T]
        if outs is None:
            outs = [self.empty_words(max(s, 1)) for s in sizes]
        h_in = (C.c_void_p * w)(*[_ptr(p) for p in planes])
        h_rows = (C.c_uint64 * m)(*[int(r) for r in rows])
        h_out = (C.c_void_p * m)(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_linear(n_bits, batch, w, h_in, h_terms, m, h_rows, int(constant), h_out, self.stream))
        return [o[:s] for o, s in zip(outs, sizes)]

    @staticmethod
    def _plain_sum_arrays(terms, planes_entries):
        """Host arrays of a csgn_uint_plain_sum shape: planes_entries[x] is the list of (cmp, k) of output plane x."""
        flat = [e for entries in planes_entries for e in entries]
        first = [0]
        for entries in planes_entries:
            first.append(first[-1] + len(entries))
        h_terms = (C.c_uint64 * max(len(terms), 1))(*[int(t) for t in terms])
        h_first = (C.c_uint64 * len(first))(*first)
        h_cmp = (C.c_int * max(len(flat), 1))(*[int(c) for c, _ in flat])
        h_k = (C.c_uint64 * max(len(flat), 1))(*[int(k) for _, k in flat])
        return h_terms, h_first, h_cmp, h_k

    def uint_plain_sum_launches(self, n_bits: int, batch: int, terms, planes_entries, constant: int = 0):
        """csgn_uint_plain_sum_launches: [unit bytes, lane items per element, plane groups, launches, elements and
        workgroups of the first launch] of a csgn_uint_plain_sum call of this shape under the calling thread's knobs."""
        h_terms, h_first, h_cmp, h_k = self._plain_sum_arrays(terms, planes_entries)
        plan = (C.c_uint64 * 6)()
        check(self.lib.csgn_uint_plain_sum_launches(n_bits, batch, len(terms), h_terms, len(planes_entries), h_first, h_cmp,
                                                    h_k, int(constant), plan))
        return [int(x) for x in plan]

    def uint_plain_sum_create(self, terms, planes_entries, constant: int = 0) -> int:
        """csgn_uint_plain_sum_create: the plan of the output planes planes_entries[x] = [(cmp, k), ...] over input
        planes of terms[j] terms per element, plus ONE in the planes whose bit of `constant` is set.  Returns the handle;
        release it with self.lib.csgn_uint_plain_sum_destroy."""
        h_terms, h_first, h_cmp, h_k = self._plain_sum_arrays(terms, planes_entries)
        handle = C.c_void_p()
        check(self.lib.csgn_uint_plain_sum_create(len(terms), h_terms, len(planes_entries), h_first, h_cmp, h_k,
                                                  int(constant), C.byref(handle)))
        return handle.value

    def uint_plain_sum_apply(self, handle: int, n_bits: int, batch: int, planes, n_out: int, outs=None):
        """csgn_uint_plain_sum of a plan over the encrypted integer `planes` (bit 0 first).  Returns the output planes,
        of csgn_uint_plain_sum_plan_terms terms per element, fresh ones unless `outs` is given."""
        dl = self.default_len(n_bits)
        T = [int(self.lib.csgn_uint_plain_sum_plan_terms(handle, x)) for x in range(n_out)]
        assert all(T), "not a plane of the plan"
        sizes = [batch * t * dl for t in T]
        if outs is None:
            outs = [self.empty_words(max(s, 1)) for s in sizes]
        assert all(o.numel() >= s for o, s in zip(outs, sizes))
        h_in = (C.c_void_p * len(planes))(*[_ptr(p) for p in planes])
        h_out = (C.c_void_p * n_out)(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_plain_sum(handle, n_bits, batch, h_in, h_out, self.stream))
        return [o[:s] for o, s in zip(outs, sizes)]

    def uint_plain_sum(self, n_bits: int, batch: int, planes, terms, planes_entries, constant: int = 0, outs=None):
        """csgn_uint_plain_sum with a plan of its own: output plane x is the sum of csgn_uint_plain(cmp, k) of `planes`
        over planes_entries[x] = [(cmp, k), ...], plus ONE where bit x of `constant` is set."""
        assert len(planes) == len(terms)
        handle = self.uint_plain_sum_create(terms, planes_entries, constant)
        try:
            outs = self.uint_plain_sum_apply(handle, n_bits, batch, planes, len(planes_entries), outs)
            torch.cuda.current_stream(self.device).synchronize()
        finally:
            self.lib.csgn_uint_plain_sum_destroy(handle)
        return outs

    @staticmethod
    def _bilinear_arrays(ta, tb, planes_pairs):
        """Host arrays of a csgn_uint_bilinear shape: planes_pairs[x] is the list of (left, right) of output plane x."""
        flat = [e for pairs in planes_pairs for e in pairs]
        first = [0]
        for pairs in planes_pairs:
            first.append(first[-1] + len(pairs))
        h_ta = (C.c_uint64 * max(len(ta), 1))(*[int(t) for t in ta])
        h_tb = (C.c_uint64 * max(len(tb), 1))(*[int(t) for t in tb])
        h_first = (C.c_uint64 * len(first))(*first)
        h_left = (C.c_uint64 * max(len(flat), 1))(*[int(i) for i, _ in flat])
        h_right = (C.c_uint64 * max(len(flat), 1))(*[int(l) for _, l in flat])
        return h_ta, h_tb, h_first, h_left, h_right

    def uint_bilinear_launches(self, n_bits: int, batch: int, ta, tb, planes_pairs, constant: int = 0):
        """csgn_uint_bilinear_launches: [unit bytes, units per element, G, tiles, workgroups per tile, launches,
        workgroups of the first launch, plane groups, staged, units a workgroup walks, operand units per element, the
        LDS budget in bytes] of a csgn_uint_bilinear call of this shape under the calling thread's knobs."""
        h_ta, h_tb, h_first, h_left, h_right = self._bilinear_arrays(ta, tb, planes_pairs)
        plan = (C.c_uint64 * 12)()
        check(self.lib.csgn_uint_bilinear_launches(n_bits, batch, len(ta), h_ta, len(tb), h_tb, len(planes_pairs), h_first,
                                                   h_left, h_right, int(constant), plan))
        return [int(x) for x in plan]

    def uint_bilinear_create(self, ta, tb, planes_pairs, constant: int = 0) -> int:
        """csgn_uint_bilinear_create: the plan of the output planes planes_pairs[x] = [(left, right), ...] over planes
        a_i of ta[i] and b_l of tb[l] terms per element, plus ONE in the planes whose bit of `constant` is set.  Returns
        the handle; release it with self.lib.csgn_uint_bilinear_destroy."""
        h_ta, h_tb, h_first, h_left, h_right = self._bilinear_arrays(ta, tb, planes_pairs)
        handle = C.c_void_p()
        check(self.lib.csgn_uint_bilinear_create(len(ta), h_ta, len(tb), h_tb, len(planes_pairs), h_first, h_left, h_right,
                                                 int(constant), C.byref(handle)))
        return handle.value

    def uint_bilinear_apply(self, handle: int, n_bits: int, batch: int, a, b, n_out: int, outs=None):
        """csgn_uint_bilinear of a plan over the encrypted integers `a` and `b` (bit 0 first).  Returns the output
        planes, of csgn_uint_bilinear_plan_terms terms per element, fresh ones unless `outs` is given."""
        dl = self.default_len(n_bits)
        T = [int(self.lib.csgn_uint_bilinear_plan_terms(handle, x)) for x in range(n_out)]
        assert all(T), "not a plane of the plan"
        sizes = [batch * t * dl for t in T]
        if outs is None:
            outs = [self.empty_words(max(s, 1)) for s in sizes]
        assert all(o.numel() >= s for o, s in zip(outs, sizes))
        h_a = (C.c_void_p * len(a))(*[_ptr(p) for p in a])
        h_b = (C.c_void_p * len(b))(*[_ptr(p) for p in b])
        h_out = (C.c_void_p * n_out)(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_bilinear(handle, n_bits, batch, h_a, h_b, h_out, self.stream))
        return [o[:s] for o, s in zip(outs, sizes)]

    def uint_bilinear(self, n_bits: int, batch: int, a, ta, b, tb, planes_pairs, constant: int = 0, outs=None):
        """csgn_uint_bilinear with a plan of its own: output plane x is the sum of a[left] * b[right] over
        planes_pairs[x] = [(left, right), ...], plus ONE where bit x of `constant` is set."""
        assert len(a) == len(ta) and len(b) == len(tb)
        handle = self.uint_bilinear_create(ta, tb, planes_pairs, constant)
        try:
            outs = self.uint_bilinear_apply(handle, n_bits, batch, a, b, len(planes_pairs), outs)
            torch.cuda.current_stream(self.device).synchronize()
        finally:
            self.lib.csgn_uint_bilinear_destroy(handle)
        return outs

    @staticmethod
    def _poly_arrays(terms, planes_monomials):
        """Host arrays of a csgn_uint_poly shape: planes_monomials[x] is the list of monomials of output plane x, each
        a sequence of input plane indices."""
        mons = [m for plane in planes_monomials for m in plane]
        first = [0]
        for plane in planes_monomials:
            first.append(first[-1] + len(plane))
        mfirst = [0]
        for m in mons:
            mfirst.append(mfirst[-1] + len(m))
        factors = [int(f) for m in mons for f in m]
        h_terms = (C.c_uint64 * max(len(terms), 1))(*[int(t) for t in terms])
        h_first = (C.c_uint64 * len(first))(*first)
        h_mfirst = (C.c_uint64 * len(mfirst))(*mfirst)
        h_factor = (C.c_uint64 * max(len(factors), 1))(*factors)
        return h_terms, h_first, h_mfirst, h_factor

    def uint_poly_launches(self, n_bits: int, batch: int, terms, planes_monomials, constant: int = 0):
        """csgn_uint_poly_launches: [unit bytes, units per element, G, tiles, workgroups per tile, launches, workgroups
        of the first launch, plane groups, staged, units a workgroup walks, operand units per element, the LDS budget in
        bytes, the monomial by division, the factor terms' mode] of a csgn_uint_poly call of this shape under the
        calling thread's knobs."""
        h_terms, h_first, h_mfirst, h_factor = self._poly_arrays(terms, planes_monomials)
        plan = (C.c_uint64 * 14)()
        check(self.lib.csgn_uint_poly_launches(n_bits, batch, len(terms), h_terms, len(planes_monomials), h_first, h_mfirst,
                                               h_factor, int(constant), plan))
        return [int(x) for x in plan]

    def uint_poly_create(self, terms, planes_monomials, constant: int = 0) -> int:
        """csgn_uint_poly_create: the plan of the output planes planes_monomials[x] = [(f1, f2, ...), ...] over input
        planes of terms[i] terms per element, plus ONE in the planes whose bit of `constant` is set.  Returns the handle;
        release it with self.lib.csgn_uint_poly_destroy."""
        h_terms, h_first, h_mfirst, h_factor = self._poly_arrays(terms, planes_monomials)
        handle = C.c_void_p()
        check(self.lib.csgn_uint_poly_create(len(terms), h_terms, len(planes_monomials), h_first, h_mfirst, h_factor,
                                             int(constant), C.byref(handle)))
        return handle.value

    def uint_poly_apply(self, handle: int, n_bits: int, batch: int, planes, n_out: int, outs=None):
        """csgn_uint_poly of a plan over the encrypted input planes.  Returns the output planes, of
        csgn_uint_poly_plan_terms terms per element, fresh ones unless `outs` is given."""
        dl = self.default_len(n_bits)
        T = [int(self.lib.csgn_uint_poly_plan_terms(handle, x)) for x in range(n_out)]
        assert all(T), "not a plane of the plan"
        sizes = [batch * t * dl for t in T]
        if outs is None:
            outs = [self.empty_words(max(s, 1)) for s in sizes]
        assert all(o.numel() >= s for o, s in zip(outs, sizes))
        h_in = (C.c_void_p * len(planes))(*[_ptr(p) for p in planes])
        h_out = (C.c_void_p * n_out)(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_poly(handle, n_bits, batch, h_in, h_out, self.stream))
        return [o[:s] for o, s in zip(outs, sizes)]

    def uint_poly(self, n_bits: int, batch: int, planes, terms, planes_monomials, constant: int = 0, outs=None):
        """csgn_uint_poly with a plan of its own: output plane x is the sum over planes_monomials[x] of the products of
        the input planes each monomial names, plus ONE where bit x of `constant` is set."""
        assert len(planes) == len(terms)
        handle = self.uint_poly_create(terms, planes_monomials, constant)
        try:
            outs = self.uint_poly_apply(handle, n_bits, batch, planes, len(planes_monomials), outs)
            torch.cuda.current_stream(self.device).synchronize()
        finally:
            self.lib.csgn_uint_poly_destroy(handle)
        return outs

    def uint_bitwise(self, n_bits: int, op: int, batch: int, a, a_terms, b=None, b_terms=None, sel=None, sel_terms: int = 0,
                     outs=None):
        """csgn_uint_bitwise: op = 1 a & b, 2 a | b, 3 a ^ b, 4 ~a, 5 sel ? a : b, 6 sel ? a : 0 of the encrypted
        integers a and b (bit 0 first; plane j a uniform batch of a_terms[j] / b_terms[j] terms) and the one-bit batch
        `sel` of sel_terms terms.  Operands the op does not read may be left out.  Returns the output planes, of
        csgn_uint_bitwise_terms terms per element, fresh ones unless `outs` is given."""
        w = len(a)
        with_b, with_sel = op in (1, 2, 3, 5), op in (5, 6)
        assert w == len(a_terms) and (not with_b or w == len(b) == len(b_terms)) and (not with_sel or sel is not None)
        h_ta = (C.c_uint64 * max(w, 1))(*[int(t) for t in a_terms])
        h_tb = (C.c_uint64 * max(w, 1))(*[int(t) for t in b_terms]) if with_b else None
        T = [int(self.lib.csgn_uint_bitwise_terms(op, int(sel_terms), int(a_terms[j]), int(b_terms[j]) if with_b else 0))
             for j in range(w)]
        assert w and all(T), "bad operation, width or term count"
        dl = self.default_len(n_bits)
        sizes = [batch * t * dl for t in T]
        if outs is None:
            outs = [self.empty_words(max(s, 1)) for s in sizes]
        h_a = (C.c_void_p * w)(*[_ptr(p) for p in a])
        h_b = (C.c_void_p * w)(*[_ptr(p) for p in b]) if with_b else None
        h_out = (C.c_void_p * w)(*[_ptr(o) for o in outs])
        check(self.lib.csgn_uint_bitwise(n_bits, op, batch, w, _ptr(sel) if with_sel else None, int(sel_terms), h_a, h_ta,
                                         h_b, h_tb, h_out, self.stream))
        return [o[:s] for o, s in zip(outs, sizes)]

    def matmul(self, n_bits: int, rows: int, inner: int, cols: int, a: torch.Tensor, t_a: int, b: torch.Tensor, t_b: int,
               transposed: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """csgn_matmul: the product over F2 of the encrypted bit matrices `a` (rows x inner, element i*inner + e, t_a
        terms each) and `b` (inner x cols, element e*cols + k, or with `transposed` cols x inner, element k*inner + e;
        t_b terms each).  Returns rows x cols elements of inner * t_a * t_b terms (a fresh tensor unless `out` is
        given)."""
        dl = self.default_len(n_bits)
        terms = int(self.lib.csgn_matmul_terms(inner, t_a, t_b))
        assert terms, "bad shape or term count"
        assert a.numel() >= rows * inner * t_a * dl and b.numel() >= inner * cols * t_b * dl
        if out is None:
            out = self.empty_words(rows * cols * terms * dl)
        assert out.numel() >= rows * cols * terms * dl
        check(self.lib.csgn_matmul(n_bits, rows, inner, cols, _ptr(a), t_a, _ptr(b), t_b, 1 if transposed else 0,
                                   _ptr(out), self.stream))
        return out[: rows * cols * terms * dl]

    def count(self, n_bits: int, count: int, group: int, t: int, ins, js, outs=None):
        """csgn_count: the bits of the number of ones among every element's `group` inputs of `t` terms each.  `ins`:
        one tensor, the grouped layout (element q * group + i), or `group` tensors of `count` elements, the plane
        layout.  `js`: the strictly ascending planes wanted.  Returns one tensor per plane, count elements of
        csgn_count_terms(group, t, j) terms (fresh ones unless `outs` is given)."""
        dl = self.default_len(n_bits)
        terms = [int(self.lib.csgn_count_terms(group, t, int(j))) for j in js]
        assert all(terms), "bad group, term count or plane"
        assert len(ins) in (1, group)
        need = (count * group if len(ins) == 1 else count) * t * dl
        assert all(x.numel() >= need for x in ins)
        if outs is None:
            outs = [self.empty_words(count * T * dl) for T in terms]
        assert all(o.numel() >= count * T * dl for o, T in zip(outs, terms))
        h_in = (C.c_void_p * len(ins))(*[_ptr(x) for x in ins])
        h_js = (C.c_uint64 * len(js))(*[int(j) for j in js])
        h_out = (C.c_void_p * len(outs))(*[_ptr(o) for o in outs])
        check(self.lib.csgn_count(n_bits, count, group, t, h_in, len(ins), len(js), h_js, h_out, self.stream))
        return [o[: count * T * dl] for o, T in zip(outs, terms)]

    def count_prefix(self, n_bits: int, count: int, group: int, t: int, ins, js, exclusive: bool = False, outs=None):
        """csgn_count_prefix: for every row r of every element's `group` inputs, the bits of the number of ones among
        the rows up to r (before r when `exclusive`).  `ins`, `js`: as in count, with 2^j <= group - exclusive.  Returns
        one block per plane (fresh ones unless `outs` is given): row r is `count` elements from term
        count * csgn_count_prefix_offset(group, t, j, exclusive, r) on, the block count * offset(.., group) terms."""
        dl = self.default_len(n_bits)
        ex = 1 if exclusive else 0
        terms = [int(self.lib.csgn_count_prefix_offset(group, t, int(j), ex, group)) for j in js]
        assert all(terms), "bad group, term count or plane"
        assert len(ins) in (1, group)
        need = (count * group if len(ins) == 1 else count) * t * dl
        assert all(x.numel() >= need for x in ins)
        if outs is None:
            outs = [self.empty_words(count * A * dl) for A in terms]
        assert all(o.numel() >= count * A * dl for o, A in zip(outs, terms))
        h_in = (C.c_void_p * len(ins))(*[_ptr(x) for x in ins])
        h_js = (C.c_uint64 * len(js))(*[int(j) for j in js])
        h_out = (C.c_void_p * len(outs))(*[_ptr(o) for o in outs])
        check(self.lib.csgn_count_prefix(n_bits, count, group, t, ex, h_in, len(ins), len(js), h_js, h_out, self.stream))
        return [o[: count * A * dl] for o, A in zip(outs, terms)]

    def wsum_create(self, ns, t: int, js) -> int:
        """csgn_wsum_create: the plan of the planes `js` (strictly ascending) for classes of ns[c] inputs of weight 2^c
        and of `t` terms each.  Returns the handle; release it with self.lib.csgn_wsum_destroy."""
        h_n = (C.c_uint64 * max(len(ns), 1))(*[int(v) for v in ns])
        h_js = (C.c_uint64 * max(len(js), 1))(*[int(j) for j in js])
        handle = C.c_void_p()
        check(self.lib.csgn_wsum_create(len(ns), h_n, t, len(js), h_js, C.byref(handle)))
        return handle.value

    def wsum_apply(self, handle: int, n_bits: int, count: int, ins, n_out: int, outs=None):
        """csgn_wsum of a plan: `ins` one tensor per class (None where the class is empty), count * ns[c] elements each,
        input i of element q at q * ns[c] + i.  Returns one tensor per plane of the plan (fresh ones unless `outs` is
        given)."""
        dl = self.default_len(n_bits)
        terms = [int(self.lib.csgn_wsum_plan_terms(handle, x)) for x in range(n_out)]
        if outs is None:
            outs = [self.empty_words(count * T * dl) for T in terms]
        assert all(o.numel() >= count * T * dl for o, T in zip(outs, terms))
        h_in = (C.c_void_p * len(ins))(*[None if x is None else _ptr(x) for x in ins])
        h_out = (C.c_void_p * len(outs))(*[_ptr(o) for o in outs])
        check(self.lib.csgn_wsum(handle, n_bits, count, h_in, h_out, self.stream))
        return [o[: count * T * dl] for o, T in zip(outs, terms)]

    def wsum(self, n_bits: int, count: int, ns, t: int, ins, js, outs=None):
        """csgn_wsum: the bits `js` of the sum of every element's inputs, ns[c] of weight 2^c and of `t` terms each in
        class c.  Returns one tensor per plane, count elements of csgn_wsum_terms(ns, t, j) terms (fresh ones unless
        `outs` is given)."""
        assert len(ins) == len(ns)
        assert all(x is None or x.numel() >= count * int(k) * t * self.default_len(n_bits) for x, k in zip(ins, ns))
        handle = self.wsum_create(ns, t, js)
        try:
            outs = self.wsum_apply(handle, n_bits, count, ins, len(js), outs)
            torch.cuda.current_stream(self.device).synchronize()
        finally:
            self.lib.csgn_wsum_destroy(handle)
        return outs

    def add_ragged(self, n_bits: int, left: torch.Tensor, off_left: torch.Tensor,
                   right: torch.Tensor, off_right: torch.Tensor,
                   total_terms_out: Optional[int] = None, max_t1: int = 0, max_t2: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """max_t1 / max_t2: upper bounds on one element's terms if the caller knows them (csgn_add_ragged_bounded)."""
        batch = off_left.numel() - 1
        dl = self.default_len(n_bits)
        if total_terms_out is None:
            total_terms_out = int(self.download(off_left[-1:])[0]) + int(self.download(off_right[-1:])[0])
        total = total_terms_out
        out = self.empty_words(max(total * dl, 1))
        off_out = self.empty_words(batch + 1)
        check(self.lib.csgn_add_ragged_bounded(n_bits, batch, max_t1, max_t2, _ptr(left), _ptr(off_left), _ptr(right),
                                               _ptr(off_right), _ptr(out), _ptr(off_out), total, self.stream))
        return out[: total * dl], off_out

    # -- decrypt ----------------------------------------------------------------------
    def decrypt_uniform(self, n_bits: int, batch: int, terms: int, words: torch.Tensor,
                        mask: torch.Tensor) -> torch.Tensor:
        bits = torch.empty(max(batch, 1), dtype=torch.uint8, device=self.device)
        scratch = torch.empty(int(self.lib.csgn_decrypt_scratch_bytes(batch, batch * terms)),
                              dtype=torch.uint8, device=self.device)
        check(self.lib.csgn_decrypt_uniform(n_bits, batch, terms, _ptr(words), _ptr(mask), _ptr(bits),
                                            _ptr(scratch), self.stream))
        return bits[:batch]

    def decrypt_ragged(self, n_bits: int, words: torch.Tensor, off: torch.Tensor,
                       mask: torch.Tensor, total_terms: Optional[int] = None, max_terms: int = 0) -> torch.Tensor:
        """max_terms: an upper bound on the terms of one ciphertext if the caller knows one (csgn_decrypt_ragged_bounded)."""
        batch = off.numel() - 1
        if total_terms is None:
            total_terms = int(self.download(off[-1:])[0])
        bits = torch.empty(max(batch, 1), dtype=torch.uint8, device=self.device)
        scratch = torch.empty(int(self.lib.csgn_decrypt_scratch_bytes(batch, total_terms)),
                              dtype=torch.uint8, device=self.device)
        check(self.lib.csgn_decrypt_ragged_bounded(n_bits, batch, total_terms, max_terms, _ptr(words), _ptr(off),
                                                   _ptr(mask), _ptr(bits), _ptr(scratch), self.stream))
        return bits[:batch]

    def uint_decrypt(self, n_bits: int, batch: int, planes, terms, mask: torch.Tensor, offsets=None, max_terms=None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """csgn_uint_decrypt: bit j of word e = Dec(element e of planes[j]), one 64-bit word per element (a fresh int64
        tensor unless `out` is given).  terms[j]: plane j's terms per element, 0 for a ragged plane, which then needs
        offsets[j] (its CSR offsets on the device, batch + 1 words) and max_terms[j] (a bound on one element's terms);
        the entries of `offsets` and `max_terms` at uniform planes are not read (None will do)."""
        w = len(planes)
        assert w == len(terms)
        ragged = [j for j in range(w) if int(terms[j]) == 0]
        h_planes = (C.c_void_p * max(w, 1))(*[None if p is None else _ptr(p) for p in planes])
        h_terms = (C.c_uint64 * max(w, 1))(*[int(t) for t in terms])
        h_off = h_total = h_max = None
        if ragged:
            assert offsets is not None and max_terms is not None
            h_off = (C.c_void_p * w)(*[_ptr(offsets[j]) if j in ragged else None for j in range(w)])
            h_total = (C.c_uint64 * w)(*[int(self.download(offsets[j][-1:])[0]) if j in ragged else 0 for j in range(w)])
            h_max = (C.c_uint64 * w)(*[int(max_terms[j]) if j in ragged else 0 for j in range(w)])
        if out is None:
            out = torch.empty(max(batch, 1), dtype=torch.int64, device=self.device)
        check(self.lib.csgn_uint_decrypt(n_bits, batch, w, h_planes, h_terms, h_off, h_total, h_max, _ptr(mask),
                                         _ptr(out), self.stream))
        return out[:batch]

    def decrypt_combined_uniform(self, n_bits: int, batch: int, t1: int, t2: int, left: torch.Tensor,
                                 right: torch.Tensor, mask: torch.Tensor, product: bool) -> torch.Tensor:
        """Dec(L*R) (product=True) or Dec(L+R) without materialising the result."""
        bits = torch.empty(max(batch, 1), dtype=torch.uint8, device=self.device)
        scratch = torch.empty(int(self.lib.csgn_decrypt_combined_scratch_bytes(batch, t1, t2)),
                              dtype=torch.uint8, device=self.device)
        fn = self.lib.csgn_decrypt_product_uniform if product else self.lib.csgn_decrypt_sum_uniform
        check(fn(n_bits, batch, t1, t2, _ptr(left), _ptr(right), _ptr(mask), _ptr(bits), _ptr(scratch),
                 self.stream))
        return bits[:batch]

    def compact_ragged(self, n_bits: int, words: torch.Tensor, off: torch.Tensor,
                       total_terms: Optional[int] = None, max_terms: int = 0,
                       out: Optional[torch.Tensor] = None, off_out: Optional[torch.Tensor] = None,
                       scratch: Optional[torch.Tensor] = None,
                       sync: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """Extension: mod-2 compaction (identical terms cancel in pairs).  Returns (terms, CSR offsets).
        max_terms: upper bound on any one ciphertext's terms if known (0 = unknown).  With sync=False
        nothing is read back and `out` is returned whole (benchmarks)."""
        batch = off.numel() - 1
        dl = self.default_len(n_bits)
        if total_terms is None:
            total_terms = int(self.download(off[-1:])[0])
        if out is None:
            out = self.empty_words(max(total_terms * dl, 1))
        if off_out is None:
            off_out = self.empty_words(batch + 1)
        if scratch is None:
            scratch = torch.empty(int(self.lib.csgn_compact_scratch_bytes(n_bits, batch, total_terms)),
                                  dtype=torch.uint8, device=self.device)
        check(self.lib.csgn_compact_ragged(n_bits, batch, total_terms, max_terms, _ptr(words), _ptr(off),
                                           _ptr(out), _ptr(off_out), _ptr(scratch), self.stream))
        if not sync:
            return out, off_out
        kept = int(self.download(off_out[-1:])[0])
        return out[: kept * dl], off_out

    # -- encrypt ----------------------------------------------------------------------
    def encrypt_explicit(self, n_bits: int, d: int, plain: torch.Tensor, rnd: torch.Tensor,
                         chosen: torch.Tensor, last: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        batch = plain.numel()
        out = self.empty_words(max(batch * self.default_len(n_bits), 1))
        check(self.lib.csgn_encrypt_explicit(n_bits, d, batch, _ptr(plain), _ptr(rnd), _ptr(chosen),
                                             _ptr(last), _ptr(mask), _ptr(out), self.stream))
        return out[: batch * self.default_len(n_bits)]

    def encrypt_device_rng(self, n_bits: int, d: int, plain: torch.Tensor, key: torch.Tensor,
                           mask: torch.Tensor, seed: int) -> torch.Tensor:
        batch = plain.numel()
        out = self.empty_words(max(batch * self.default_len(n_bits), 1))
        check(self.lib.csgn_encrypt_device_rng(n_bits, d, batch, _ptr(plain), _ptr(key), _ptr(mask),
                                               seed & (2**64 - 1), _ptr(out), self.stream))
        return out[: batch * self.default_len(n_bits)]

    def rng_from_seed(self, seed: int, rounds: int = 8) -> "capi.CsgnRng":
        r = capi.CsgnRng()
        check(self.lib.csgn_rng_from_seed(C.byref(r), seed & (2**64 - 1), rounds))
        return r

    def rng_from_os(self, rounds: int = 8) -> "capi.CsgnRng":
        r = capi.CsgnRng()
        check(self.lib.csgn_rng_from_os(C.byref(r), rounds))
        return r

    def encrypt_keyed(self, n_bits: int, d: int, plain: torch.Tensor, key: torch.Tensor, mask: torch.Tensor,
                      rng: "capi.CsgnRng", first_ciphertext: int = 0,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Keyed (ChaCha) device-generator encrypt; ciphertext i draws stream position first_ciphertext + i."""
        batch = plain.numel()
        dl = self.default_len(n_bits)
        if out is None:
            out = self.empty_words(max(batch * dl, 1))
        check(self.lib.csgn_encrypt_keyed(n_bits, d, batch, first_ciphertext, _ptr(plain), _ptr(key), _ptr(mask),
                                          C.byref(rng), _ptr(out), self.stream))
        return out[: batch * dl]

    def encrypt_mul_keyed(self, n_bits: int, d: int, plain_a: torch.Tensor, plain_b: torch.Tensor, key: torch.Tensor,
                          mask: torch.Tensor, rng_a: "capi.CsgnRng", rng_b: "capi.CsgnRng", first_ciphertext: int = 0,
                          with_bits: bool = True):
        """Fused fresh chain: product b = Enc_A(plain_a[b]) & Enc_B(plain_b[b]) in one kernel
        (csgn_encrypt_mul_keyed); returns (products, Dec bits or None)."""
        batch = plain_a.numel()
        assert plain_b.numel() == batch
        dl = self.default_len(n_bits)
        out = self.empty_words(max(batch * dl, 1))
        bits = torch.full((max(batch, 1),), 7, dtype=torch.uint8, device=self.device) if with_bits else None
        check(self.lib.csgn_encrypt_mul_keyed(n_bits, d, batch, first_ciphertext, _ptr(plain_a), _ptr(plain_b), _ptr(key),
                                              _ptr(mask), C.byref(rng_a), C.byref(rng_b), _ptr(out), _ptr(bits),
                                              self.stream))
        return out[: batch * dl], (bits[:batch] if with_bits else None)

    # -- permutation --------------------------------------------------------------------
    def permute_uniform(self, n_bits: int, batch: int, terms_in: int, words: torch.Tensor,
                        perm: torch.Tensor, per_term: bool = False) -> torch.Tensor:
        dl = self.default_len(n_bits)
        n_out = batch * (terms_in if per_term else 1) * dl
        out = self.empty_words(max(n_out, 1))
        check(self.lib.csgn_permute_uniform(n_bits, batch, terms_in, int(per_term), _ptr(words),
                                            _ptr(perm), _ptr(out), self.stream))
        return out[:n_out]

    # -- explicit bitlen (one ciphertext) ------------------------------------------------
    def decrypt_bitlen(self, n_bits: int, key: torch.Tensor, words: torch.Tensor, bitlen: torch.Tensor) -> int:
        length = words.numel()
        bit = torch.zeros(1, dtype=torch.uint8, device=self.device)
        scratch = torch.empty(int(self.lib.csgn_bitlen_scratch_bytes(length)), dtype=torch.uint8, device=self.device)
        check(self.lib.csgn_decrypt_bitlen(n_bits, key.numel(), length, _ptr(words), _ptr(bitlen), _ptr(key),
                                           _ptr(bit), _ptr(scratch), self.stream))
        return int(bit.item())

    def permute_bitlen(self, n_bits: int, words: torch.Tensor, bitlen: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
        length = words.numel()
        out = self.empty_words(self.default_len(n_bits))
        scratch = torch.empty(int(self.lib.csgn_bitlen_scratch_bytes(length)), dtype=torch.uint8, device=self.device)
        check(self.lib.csgn_permute_bitlen(n_bits, length, _ptr(words), _ptr(bitlen), _ptr(perm), _ptr(out),
                                           _ptr(scratch), self.stream))
        return out

    # -- harness --------------------------------------------------------------------------
    def synth_fill(self, seed: int, n_bits: int, first_word: int, n_words: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if out is None:
            out = self.empty_words(n_words)
        check(self.lib.csgn_synth_fill(seed & (2**64 - 1), n_bits, first_word, n_words, _ptr(out),
                                       self.stream))
        return out

    def digest(self, words: torch.Tensor, n_words: Optional[int] = None, first_index: int = 0) -> int:
        if n_words is None:
            n_words = words.numel()
        acc = torch.zeros(1, dtype=torch.int64, device=self.device)
        check(self.lib.csgn_digest(_ptr(words), n_words, first_index, _ptr(acc), self.stream))
        return int(acc.item()) & (2**64 - 1)

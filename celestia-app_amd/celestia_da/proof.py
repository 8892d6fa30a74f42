"""Mirror of pkg/proof (ShareProof, NewShareInclusionProofFromEDS) and
pkg/inclusion GetCommitment over a device-resident square (libcda.so).

Reference: pkg/proof/proof.go:22-206 (NewTxInclusionProof,
NewShareInclusionProof, NewShareInclusionProofFromEDS), pkg/proof/proof.pb.go (ShareProof,
RowProof, NMTProof, Proof field names), pkg/inclusion/get_commit.go:12-30.
The square is extended once (`ResidentSquare`); the EDS, every row-tree
level and the data-root tree stay in HBM, so each proof is a gather; the
proofs of many ranges come from one launch as the flat batch the verifier
takes (`ResidentSquare.share_proofs_batch`, `ShareProofsBatch`).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import NMT_ROOT_SIZE, SHARE_SIZE, default_context, ptr


@dataclass
class NMTProof:                     # proof.pb.go NMTProof
    start: int
    end: int
    nodes: list
    leaf_hash: bytes = b""


@dataclass
class Proof:                        # go-square/merkle Proof (RowProof.Proofs)
    total: int
    index: int
    leaf_hash: bytes
    aunts: list


ERR_ROW_PROOF = "row proof failed to verify"        # row_proof.go:22
ERR_SHARE_PROOF = "share proof failed to verify"    # share_proof.go:48


@dataclass
class RowProof:
    row_roots: list
    proofs: list
    start_row: int
    end_row: int

    def structural_error(self):
        """RowProof.Validate's count checks (row_proof.go:15-20): the error
        text, or None.  No GPU."""
        rows = self.end_row - self.start_row + 1
        if rows != len(self.row_roots):
            return f"the number of rows {rows} must equal the number of row roots {len(self.row_roots)}"
        if len(self.proofs) != len(self.row_roots):
            return f"the number of proofs {len(self.proofs)} must equal the number of row roots {len(self.row_roots)}"
        return None

    def validate(self, root: bytes, ctx=None):
        """RowProof.Validate(root) (row_proof.go:13-27): None, or ValueError
        with the reference's text.  The merkle proofs are verified on the GPU
        (cda_share_proofs_verify, row half only)."""
        err = self.structural_error()
        if err is None and self.row_roots:
            n = len(self.row_roots[0])
            # (a namespace longer than the library's bound is the call's CDA_ERR_INVALID, not a verdict)
            ok = n >= 34 and (n - 32) % 2 == 0 and len(root) == 32 \
                and all(len(r) == n for r in self.row_roots) and all(_proof_well_formed(q) for q in self.proofs)
            if ok:
                segs = [(0, 1, [], r, q) for r, q in zip(self.row_roots, self.proofs)]
                ok = _verify_batch(ctx, (n - 32) // 2, 0, [(bytes((n - 32) // 2), bytes(root), segs, [])],
                                   rows=True, nmt=False)[0] == 0
            if not ok:
                err = ERR_ROW_PROOF
        if err is not None:
            raise ValueError(err)


@dataclass
class ShareProof:
    data: list
    share_proofs: list
    namespace_id: bytes
    row_proof: RowProof
    namespace_version: int = 0
    extra: dict = field(default_factory=dict)

    def structural_error(self):
        """The checks of ShareProof.Validate that come before the row proof
        (share_proof.go:17-41) followed by RowProof.Validate's count checks,
        in the reference's order: the error text, or None.  No GPU."""
        if not self.data:
            return "empty share proof"
        n_in_proofs = sum(p.end - p.start for p in self.share_proofs)
        rp = self.row_proof
        if len(self.share_proofs) != len(rp.row_roots):
            return (f"the number of share proofs {len(self.share_proofs)} must equal the number of row roots "
                    f"{len(rp.row_roots)}")
        if len(self.data) != n_in_proofs:
            return (f"the number of shares {len(self.data)} must equal the number of shares in share proofs "
                    f"{n_in_proofs}")
        for p in self.share_proofs:
            if p.start < 0:
                return "proof index cannot be negative"
            if p.end - p.start <= 0:
                return "proof total must be positive"
        return rp.structural_error()

    def validate(self, root: bytes, ctx=None):
        """ShareProof.Validate(root) (share_proof.go:16-52): None, or
        ValueError with the reference's text, in the reference's order of
        checks.  The structural checks need no GPU; the row proofs and the NMT
        inclusion proofs are verified on it in one cda_share_proofs_verify call."""
        err = validate_share_proofs([self], [root], ctx)[0]
        if err is not None:
            raise ValueError(err)

    def verify_proof(self, ctx=None) -> bool:
        """ShareProof.VerifyProof (share_proof.go:54-82): the NMT inclusion
        proofs of the shares against the proof's own row roots (no data root)."""
        if len(self.share_proofs) != len(self.row_proof.row_roots) or any(
                p.start < 0 or p.end <= p.start for p in self.share_proofs) or len(self.data) != sum(
                p.end - p.start for p in self.share_proofs):
            return False
        if not self.share_proofs:
            return True
        if not _nmt_well_formed(self):
            return False
        ns = bytes([self.namespace_version]) + bytes(self.namespace_id)
        segs = [(p.start, p.end, p.nodes, r, None) for p, r in zip(self.share_proofs, self.row_proof.row_roots)]
        return _verify_batch(ctx, len(ns), len(self.data[0]), [(ns, None, segs, self.data)],
                             rows=False, nmt=True)[0] == 0


def _log2(x: int) -> int:
    n = 0
    while (1 << n) < x:
        n += 1
    return n


class ResidentSquare:
    """An extended square kept on the GPU (cda_square_*)."""

    def __init__(self, ods, ctx=None):
        self.ctx = ctx or default_context()
        a = np.ascontiguousarray(np.asarray(ods, dtype=np.uint8).reshape(-1, SHARE_SIZE))
        self.h = C.c_void_p()
        rc = self.ctx.lib.cda_square_create(self.ctx.h, ptr(a), a.shape[0], C.byref(self.h))
        self.push_order_error = rc == _lib.CDA_ERR_PUSH_ORDER
        if rc not in (_lib.CDA_OK, _lib.CDA_ERR_PUSH_ORDER):
            self.ctx.check(rc)
        k = C.c_uint32()
        self.ctx.check(self.ctx.lib.cda_square_dah(self.h, C.byref(k), None, None, None, None))
        self.k = k.value

    @classmethod
    def _borrowed(cls, owner: "ResidentSquareSet", handle, push_order_error: bool) -> "ResidentSquare":
        """A member of a ResidentSquareSet (cda_square_set_at): the handle is
        the set's, and the object keeps the set alive."""
        sq = object.__new__(cls)
        sq.ctx, sq.h, sq.k, sq.owner = owner.ctx, handle, owner.k, owner
        sq.push_order_error = push_order_error
        return sq

    def close(self):
        if getattr(self, "h", None):
            if getattr(self, "owner", None) is None:   # a member's handle ends with its set
                self.ctx.lib.cda_square_destroy(self.h)
            self.h = None
            self.owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dah(self):
        """(row_roots, col_roots, data_root)."""
        W = 2 * self.k
        rows = np.empty(W * NMT_ROOT_SIZE, dtype=np.uint8)
        cols = np.empty(W * NMT_ROOT_SIZE, dtype=np.uint8)
        root = np.empty(32, dtype=np.uint8)
        self.ctx.check(self.ctx.lib.cda_square_dah(self.h, None, ptr(rows), ptr(cols), ptr(root), None))
        split = lambda b: [b[i * NMT_ROOT_SIZE:(i + 1) * NMT_ROOT_SIZE].tobytes() for i in range(W)]  # noqa: E731
        return split(rows), split(cols), root.tobytes()

    def eds(self) -> np.ndarray:
        W = 2 * self.k
        out = np.empty(W * W * SHARE_SIZE, dtype=np.uint8)
        self.ctx.check(self.ctx.lib.cda_square_dah(self.h, None, None, None, None, ptr(out)))
        return out.reshape(W, W, SHARE_SIZE)

    def share_proof(self, namespace: bytes, start: int, end: int) -> ShareProof:
        """proof.NewShareInclusionProofFromEDS(eds, namespace, shares.Range{start, end})."""
        k = self.k
        if not (0 <= start < end <= k * k):
            raise _lib.CdaError(_lib.CDA_ERR_INVALID, "share range out of the original square")
        W = 2 * k
        R = (end - 1) // k - start // k + 1
        M, A = 2 * _log2(W), _log2(2 * W)
        shares = np.empty((end - start) * SHARE_SIZE, dtype=np.uint8)
        ns, ne = (C.c_int32 * R)(), (C.c_int32 * R)()
        cnt = (C.c_uint32 * R)()
        nodes = np.empty(R * M * NMT_ROOT_SIZE, dtype=np.uint8)
        roots = np.empty(R * NMT_ROOT_SIZE, dtype=np.uint8)
        leaf = np.empty(R * 32, dtype=np.uint8)
        aunts = np.empty(R * A * 32, dtype=np.uint8)
        r0, r1 = C.c_uint32(), C.c_uint32()
        self.ctx.check(self.ctx.lib.cda_square_share_proof(self.h, start, end, ptr(shares), C.byref(r0), C.byref(r1),
                                                           ns, ne, cnt, ptr(nodes), ptr(roots), ptr(leaf),
                                                           ptr(aunts)))
        nb, rb, lb, ab = nodes.tobytes(), roots.tobytes(), leaf.tobytes(), aunts.tobytes()
        sp = [NMTProof(ns[i], ne[i], [nb[(i * M + q) * 90:(i * M + q + 1) * 90] for q in range(cnt[i])])
              for i in range(R)]
        proofs = [Proof(2 * W, r0.value + i, lb[32 * i:32 * (i + 1)],
                        [ab[(i * A + q) * 32:(i * A + q + 1) * 32] for q in range(A)]) for i in range(R)]
        sb = shares.tobytes()
        return ShareProof(data=[sb[i * SHARE_SIZE:(i + 1) * SHARE_SIZE] for i in range(end - start)],
                          share_proofs=sp, namespace_id=bytes(namespace[1:]),
                          row_proof=RowProof([rb[90 * i:90 * (i + 1)] for i in range(R)], proofs, r0.value, r1.value),
                          namespace_version=namespace[0])

    def share_proofs_batch(self, ranges, out=None) -> "ShareProofsBatch":
        """NewShareInclusionProofFromEDS for every (start, end) of `ranges` in
        one cda_square_share_proofs call (one launch): a ShareProofsBatch.
        out: a ShareProofsBatch.empty(k, ranges) to fill instead of a new one."""
        r = _ranges_array(ranges)
        if out is None:
            out = ShareProofsBatch.empty(self.k, r)
        starts, ends = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
        u32p = C.POINTER(C.c_uint32)
        o = out.out_struct()
        self.ctx.check(self.ctx.lib.cda_square_share_proofs(self.h, starts.ctypes.data_as(u32p),
                                                            ends.ctypes.data_as(u32p), len(r), C.byref(o)))
        return out

    def sample_proofs(self, coords, out=None):
        """Data-availability samples of the EDS (cda_square_sample_proofs):
        coords is an (n, 3) integer array of (row, col, axis), 0 <= row, col <
        2k, axis 0 = against the row root, 1 = against the column root (an
        (n, 2) array: all on the row axis).  One launch for the whole batch;
        returns a sampling.SampleBatch."""
        from . import sampling
        return sampling.sample_proofs(self, coords, out)

    def axis_halves(self, coords):
        """Half rows / half columns of the EDS (cda_square_axis_halves): coords
        is an (n, 3) integer array of (axis, index, side); returns an
        axis_halves.HalfBatch."""
        from . import axis_halves
        return axis_halves.serve(self, coords)

    def namespace_proofs(self, namespaces, out=None):
        """All shares of every 29-byte namespace of `namespaces` with nmt
        ProveNamespace's proofs, absence proofs included, the rows chosen as
        GetSharesByNamespace chooses them (cda_square_namespace_plan /
        _proofs): a namespace.NamespaceProofsBatch."""
        from . import namespace
        return namespace.namespace_proofs(self, namespaces, out)

    def blob_commitments(self, starts, share_lens, subtree_root_threshold: int = 64):
        """inclusion.GetCommitment for each (start, share_len)."""
        n = len(starts)
        s = (C.c_uint32 * max(1, n))(*starts)
        ln = (C.c_uint32 * max(1, n))(*share_lens)
        out = np.empty(32 * max(1, n), dtype=np.uint8)
        self.ctx.check(self.ctx.lib.cda_square_blob_commitments(self.h, s, ln, n, subtree_root_threshold, ptr(out)))
        b = out.tobytes()
        return [b[32 * i:32 * (i + 1)] for i in range(n)]

    def commitment_proofs(self, starts, share_lens, subtree_root_threshold: int = 64, out=None):
        """The blob commitment proof of every blob (start, share_len) in one
        cda_square_commitment_proofs call (one launch, one more for the
        commitments): a CommitmentProofsBatch.  out: a
        CommitmentProofsBatch.empty(k, starts, share_lens, threshold) to fill."""
        st, ln = _u32_array(starts, "start"), _u32_array(share_lens, "share_len")
        if len(st) != len(ln):
            raise ValueError(f"{len(st)} starts but {len(ln)} share_lens")
        if out is None:
            out = CommitmentProofsBatch.empty(self.k, st, ln, subtree_root_threshold)
        u32p = C.POINTER(C.c_uint32)
        o = out.out_struct()
        self.ctx.check(self.ctx.lib.cda_square_commitment_proofs(self.h, st.ctypes.data_as(u32p), ln.ctypes.data_as(u32p),
                                                                 len(st), subtree_root_threshold, C.byref(o)))
        return out

    @staticmethod
    def _ranges_args(ranges):
        """(starts, ends, n, the arrays behind the pointers) for cda_square_parse*; None: the whole square."""
        if ranges is None:
            return None, None, 0, None
        r = _ranges_array(ranges)
        if len(r) == 0:   # no range is nothing to parse, not the whole square
            raise _lib.CdaError(_lib.CDA_ERR_INVALID, "no share range given")
        st, en = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
        u32p = C.POINTER(C.c_uint32)
        return st.ctypes.data_as(u32p), en.ctypes.data_as(u32p), len(r), (st, en)

    def parse_plan(self, ranges=None) -> dict:
        """cda_square_parse_plan: the counts and byte sizes of what the square
        (or its share ranges `ranges`, [(start, end)]) parses to."""
        from . import shares
        st, en, n, _alive = self._ranges_args(ranges)
        p = _lib.ParsePlanT()
        self.ctx.check(self.ctx.lib.cda_square_parse_plan(self.h, st, en, n, C.byref(p)))
        return shares.plan_dict(p)

    def parse(self, ranges=None, blob_data: bool = True):
        """go-square shares.ParseShares of the original square, or of its share
        ranges `ranges` ([(start, end)], ascending and disjoint, each parsed as
        an input of its own), on the GPU (cda_square_parse_plan, then
        cda_square_parse): a shares.ParsedSquare with the txs, the PFBs' raw
        IndexWrapper bytes, the blobs with their starts and share counts and
        the units' share ranges.  blob_data=False: the table only, the blobs'
        data stays empty."""
        from . import shares
        st, en, n, _alive = self._ranges_args(ranges)
        p = _lib.ParsePlanT()
        self.ctx.check(self.ctx.lib.cda_square_parse_plan(self.h, st, en, n, C.byref(p)))
        buf = shares.ParseBuffers(p, blob_data=blob_data)
        o = buf.out_struct()
        self.ctx.check(self.ctx.lib.cda_square_parse(self.h, st, en, n, C.byref(o)))
        return buf.parsed()

    def subtree_root(self, row: int, walk) -> bytes:
        """EDSSubTreeRootCacher.getSubTreeRoot (pkg/inclusion/nmt_caching.go:111-124):
        the node of EDS row tree `row` reached by `walk` (False = WalkLeft,
        True = WalkRight) from its root."""
        w = np.array([1 if x else 0 for x in walk] or [0], dtype=np.uint8)
        out = np.empty(90, dtype=np.uint8)
        self.ctx.check(self.ctx.lib.cda_square_subtree_root(self.h, row, ptr(w), len(walk), ptr(out)))
        return out.tobytes()


class ResidentSquareSet:
    """n extended squares of one width kept on the GPU, built in one
    submission (cda_square_set_*): from host arrays (from_ods, from_eds) or
    from a batch already in HBM (from_device_ods, from_device_eds) -- the output
    of Context.extend_dah_device, replay or rsmt2d.repair_batch_device.
    `set[i]` is a ResidentSquare that borrows from the set and keeps it alive;
    sampling.sample_proofs_set answers samples of many members in one launch.

    An EDS source is hashed as it is (no Reed-Solomon work, the parity is not
    checked): compare dah()'s data roots with the ones you trust.  A square
    whose ODS is out of push order stays in the set with its blind roots:
    `status[i]` is CDA_ERR_PUSH_ORDER and `push_order_error` is set."""

    def __init__(self, ctx, handle, rc):
        import weakref
        self.ctx, self.h = ctx, handle
        self.push_order_error = rc == _lib.CDA_ERR_PUSH_ORDER
        k, n = C.c_uint32(), C.c_uint32()
        self.ctx.check(self.ctx.lib.cda_square_set_info(self.h, C.byref(k), C.byref(n)))
        self.k, self.n = k.value, n.value
        self._members = weakref.WeakSet()
        self.status = np.zeros(self.n, dtype=np.int32)
        self.ctx.check(self.ctx.lib.cda_square_set_dah(self.h, None, None, None,
                                                       self.status.ctypes.data_as(C.POINTER(C.c_int32))))

    @classmethod
    def _create(cls, ctx, src, d_src, kind, k, n, stream=None):
        ctx = ctx or default_context()
        h = C.c_void_p()
        if d_src is None:
            rc = ctx.lib.cda_square_set_create(ctx.h, ptr(src), kind, k, n, C.byref(h))
        else:
            rc = ctx.lib.cda_square_set_create_device(ctx.h, d_src, kind, k, n, stream, C.byref(h))
        if rc not in (_lib.CDA_OK, _lib.CDA_ERR_PUSH_ORDER):
            ctx.check(rc)
        return cls(ctx, h, rc)

    @staticmethod
    def _host_batch(a, eds: bool):
        """(contiguous uint8 array, k, n) of a batch of squares: (n, w, w, 512), (n, w*w, 512) or (n, w*w*512)."""
        a = np.ascontiguousarray(np.asarray(a, dtype=np.uint8))
        if a.ndim < 2 or a.shape[0] == 0:
            raise ValueError("a batch of squares has the shape (n, ...) with n >= 1")
        n = a.shape[0]
        cells = a[0].size // SHARE_SIZE
        w = 1
        while w * w < cells:
            w *= 2
        if w * w * SHARE_SIZE != a[0].size or (eds and w < 2):
            raise ValueError(f"{a[0].size} bytes per square are no square of 512-byte shares")
        return a, (w // 2 if eds else w), n

    @classmethod
    def from_ods(cls, ods, ctx=None) -> "ResidentSquareSet":
        """n original squares on the host: extended and hashed in one submission."""
        a, k, n = cls._host_batch(ods, False)
        return cls._create(ctx, a, None, _lib.CDA_SET_FROM_ODS, k, n)

    @classmethod
    def from_eds(cls, eds, ctx=None) -> "ResidentSquareSet":
        """n extended squares on the host: hashed as they are."""
        a, k, n = cls._host_batch(eds, True)
        return cls._create(ctx, a, None, _lib.CDA_SET_FROM_EDS, k, n)

    @staticmethod
    def _device_ptr(d, nbytes: int) -> int:
        if hasattr(d, "data_ptr"):
            if not d.is_contiguous() or d.numel() * d.element_size() != nbytes:
                raise ValueError(f"the tensor must hold {nbytes} contiguous bytes")
            d = d.data_ptr()
        return int(d)

    @classmethod
    def from_device_ods(cls, d_ods, k: int, n: int, stream=None, ctx=None) -> "ResidentSquareSet":
        """n original squares in HBM (a device pointer or anything with
        data_ptr, n * k * k * 512 contiguous bytes, 16-byte aligned), read
        only; the work is ordered after `stream` (None: the null stream)."""
        return cls._create(ctx, None, cls._device_ptr(d_ods, n * k * k * SHARE_SIZE), _lib.CDA_SET_FROM_ODS, k, n,
                           stream)

    @classmethod
    def from_device_eds(cls, d_eds, k: int, n: int, stream=None, ctx=None) -> "ResidentSquareSet":
        """n extended squares in HBM (n * (2k)^2 * 512 contiguous bytes), copied
        and hashed as they are; as from_device_ods otherwise."""
        return cls._create(ctx, None, cls._device_ptr(d_eds, n * 4 * k * k * SHARE_SIZE), _lib.CDA_SET_FROM_EDS, k,
                           n, stream)

    def __len__(self) -> int:
        return self.n

    def __getitem__(self, i: int) -> ResidentSquare:
        if not self.h:
            raise _lib.CdaError(_lib.CDA_ERR_INVALID, "the square set is closed")
        i = int(i)
        if i < 0:
            i += self.n
        if not 0 <= i < self.n:
            raise IndexError(f"square {i} of a set of {self.n}")
        m = C.c_void_p()
        self.ctx.check(self.ctx.lib.cda_square_set_at(self.h, i, C.byref(m)))
        sq = ResidentSquare._borrowed(self, m, self.status[i] == _lib.CDA_ERR_PUSH_ORDER)
        self._members.add(sq)
        return sq

    def dah(self):
        """(row_roots, col_roots, data_roots) as uint8 arrays of shape (n, 2k, 90), (n, 2k, 90) and (n, 32)."""
        W = 2 * self.k
        rows = np.empty((self.n, W, NMT_ROOT_SIZE), dtype=np.uint8)
        cols = np.empty((self.n, W, NMT_ROOT_SIZE), dtype=np.uint8)
        roots = np.empty((self.n, 32), dtype=np.uint8)
        self.ctx.check(self.ctx.lib.cda_square_set_dah(self.h, ptr(rows), ptr(cols), ptr(roots), None))
        return rows, cols, roots

    def sample_proofs(self, coords, out=None):
        """sampling.sample_proofs_set(self, coords, out)."""
        from . import sampling
        return sampling.sample_proofs_set(self, coords, out)

    def axis_halves(self, coords):
        """axis_halves.serve_set(self, coords): coords (n, 4) of (square, axis, index, side)."""
        from . import axis_halves
        return axis_halves.serve_set(self, coords)

    def namespace_plan(self, queries) -> dict:
        """cda_square_set_namespace_plan: the sizes of the answer to `queries`,
        rows of (square, 29-byte namespace)."""
        from . import namespace
        return namespace.namespace_plan_set(self, queries)

    def namespace_proofs(self, queries, out=None):
        """ResidentSquare.namespace_proofs across the set
        (cda_square_set_namespace_proofs): `queries` are rows of (square,
        namespace) of any number of members, answered in the launches of one
        square's call.  Returns a namespace.SetNamespaceProofs: the flat
        NamespaceProofsBatch in request order plus the squares column."""
        from . import namespace
        return namespace.namespace_proofs_set(self, queries, out)

    def share_proofs_batch(self, ranges, out=None) -> "SetShareProofs":
        """ResidentSquare.share_proofs_batch across the set
        (cda_square_set_share_proofs, one launch): `ranges` are rows of
        (square, start, end).  out: a ShareProofsBatch.empty(k, ranges[:, 1:])
        to fill instead of a new one."""
        r = np.asarray(ranges, dtype=np.int64).reshape(-1, 3)
        if r.size and (r[:, 0].min() < 0 or r[:, 0].max() >= 1 << 32):
            raise _lib.CdaError(_lib.CDA_ERR_INVALID, "square out of range")
        rr = _ranges_array(r[:, 1:])
        if out is None:
            out = ShareProofsBatch.empty(self.k, rr)
        squares = np.ascontiguousarray(r[:, 0], dtype=np.uint32)
        starts, ends = np.ascontiguousarray(rr[:, 0]), np.ascontiguousarray(rr[:, 1])
        u32p = C.POINTER(C.c_uint32)
        o = out.out_struct()
        self.ctx.check(self.ctx.lib.cda_square_set_share_proofs(self.h, squares.ctypes.data_as(u32p),
                                                                starts.ctypes.data_as(u32p),
                                                                ends.ctypes.data_as(u32p), len(rr), C.byref(o)))
        return SetShareProofs(out, squares)

    def close(self):
        """Ends the set and its members: a ResidentSquare taken from it is closed too."""
        if getattr(self, "h", None):
            for sq in list(self._members):
                sq.h, sq.owner = None, None
            self.ctx.lib.cda_square_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------- proofs of many ranges at once
def _ranges_array(ranges) -> np.ndarray:
    """(n, 2) uint32 array of (start, end)."""
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    if r.size and (r.min() < 0 or r.max() >= 1 << 32):
        raise _lib.CdaError(_lib.CDA_ERR_INVALID, "share range out of the original square")
    return r.astype(np.uint32)


def share_proofs_plan(k: int, ranges) -> dict:
    """cda_square_share_proofs_plan: the sizes of the batch of `ranges` of a
    square of ODS width k -- n_segments, n_nodes, n_aunts, aunts_per_segment,
    n_shares.  Host only, no context; CdaError names the range and the field."""
    r = _ranges_array(ranges)
    L = _lib.load()
    starts, ends = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
    u32p = C.POINTER(C.c_uint32)
    p = _lib.ShareProofsPlanT()
    rc = L.cda_square_share_proofs_plan(k, starts.ctypes.data_as(u32p), ends.ctypes.data_as(u32p), len(r), C.byref(p))
    if rc != _lib.CDA_OK:
        raise _lib.CdaError(rc, L.cda_last_error(None).decode())
    return {n: getattr(p, n) for n, _ in _lib.ShareProofsPlanT._fields_}


class ShareProofsBatch:
    """The share proofs of n ranges of one square as the flat arrays of
    cda_share_proofs_out (numpy; include/cda.h): proof i owns the segments
    (rows) seg_off[i] .. seg_off[i + 1], segment g the nodes node_off[g] ..
    node_off[g + 1] and the aunts aunt_off[g] .. aunt_off[g + 1]; the shares
    are concatenated in proof then segment order."""

    FIELDS = ("seg_off", "nmt_start", "nmt_end", "node_off", "nodes", "row_roots", "rfc_total", "rfc_index",
              "rfc_leaf_hash", "aunt_off", "aunts", "shares", "namespaces", "start_row", "end_row", "one_namespace")

    def __init__(self, k, ranges, **arrays):
        self.k, self.ranges = k, ranges
        for name in self.FIELDS:
            setattr(self, name, arrays[name])

    @classmethod
    def empty(cls, k, ranges, fill=None):
        """Buffers of the plan's sizes (filled with the byte `fill` if given)."""
        r = _ranges_array(ranges)
        p = share_proofs_plan(k, r)
        n, S = len(r), p["n_segments"]
        shapes = {"seg_off": ((n + 1,), np.uint32), "nmt_start": ((S,), np.int32), "nmt_end": ((S,), np.int32),
                  "node_off": ((S + 1,), np.uint32), "nodes": ((p["n_nodes"], NMT_ROOT_SIZE), np.uint8),
                  "row_roots": ((S, NMT_ROOT_SIZE), np.uint8), "rfc_total": ((S,), np.int64),
                  "rfc_index": ((S,), np.int64), "rfc_leaf_hash": ((S, 32), np.uint8),
                  "aunt_off": ((S + 1,), np.uint32), "aunts": ((p["n_aunts"], 32), np.uint8),
                  "shares": ((p["n_shares"], SHARE_SIZE), np.uint8), "namespaces": ((n, 29), np.uint8),
                  "start_row": ((n,), np.uint32), "end_row": ((n,), np.uint32), "one_namespace": ((n,), np.uint8)}
        arrays = {}
        for name, (shape, dtype) in shapes.items():
            a = np.empty(shape, dtype=dtype)
            if fill is not None:
                a.view(np.uint8).fill(fill)
            arrays[name] = a
        return cls(k, r, **arrays)

    def __len__(self):
        return len(self.ranges)

    def arrays(self):
        return tuple(getattr(self, name) for name in self.FIELDS)

    def out_struct(self, skip=()):
        """cda_share_proofs_out over the arrays (NULL for the names in `skip`)."""
        o = _lib.ShareProofsOut()
        for (name, t), a in zip(_lib.ShareProofsOut._fields_, self.arrays()):
            assert name in self.FIELDS
            if name not in skip:
                setattr(o, name, a.ctypes.data_as(t))
        return o

    def batch(self, data_root):
        """The cda_share_proof_batch for cda_share_proofs_verify over these
        arrays, unchanged: pointer assignment, no per-proof objects.
        data_root: 32 bytes for every proof, or n * 32."""
        n = len(self)
        roots = np.frombuffer(bytes(data_root), dtype=np.uint8) if isinstance(data_root, (bytes, bytearray)) \
            else np.ascontiguousarray(data_root, dtype=np.uint8).reshape(-1)
        if roots.size == 32:
            roots = np.tile(roots, max(1, n))
        if roots.size != 32 * max(1, n):
            raise ValueError(f"{n} proofs but {roots.size} bytes of data roots")
        b = _lib.ShareProofBatch()
        b.n_proofs, b.ns_len, b.share_len = n, 29, SHARE_SIZE
        b.data_roots = roots.ctypes.data_as(_lib.ShareProofBatch._u8p)
        for name, t in _lib.ShareProofBatch._fields_:
            if name in self.FIELDS:
                setattr(b, name, getattr(self, name).ctypes.data_as(t))
        b.n_nodes, b.n_aunts, b.n_shares = len(self.nodes), len(self.aunts), len(self.shares)
        b._keep = (roots, self)   # the struct borrows the arrays
        return b

    def verify(self, data_root, ctx=None) -> np.ndarray:
        """cda_share_proofs_verify of the batch: verdict per proof (0 valid, 1
        row proof, 2 share proof)."""
        ctx = ctx or default_context()
        b = self.batch(data_root)
        verdict = np.full(max(1, len(self)), 255, dtype=np.uint8)
        ctx.check(ctx.lib.cda_share_proofs_verify(ctx.h, C.byref(b), ptr(verdict)))
        return verdict[:len(self)]

    def proofs(self, namespaces=None) -> list:
        """One ShareProof per range, equal field for field to
        ResidentSquare.share_proof(namespace, start, end).  namespaces: one
        29-byte namespace per range; None takes the first share's, and a range
        whose shares carry more than one namespace raises ParseNamespace's
        error (ValueError), computed from the returned shares."""
        W = 2 * self.k
        nb, rb, lb, ab, sb = (a.tobytes() for a in (self.nodes, self.row_roots, self.rfc_leaf_hash, self.aunts,
                                                    self.shares))
        seg_off, node_off, aunt_off = self.seg_off.tolist(), self.node_off.tolist(), self.aunt_off.tolist()
        st, en, idx = self.nmt_start.tolist(), self.nmt_end.tolist(), self.rfc_index.tolist()
        r0, r1 = self.start_row.tolist(), self.end_row.tolist()
        cut = lambda b, lo, hi, sz: [b[i * sz:(i + 1) * sz] for i in range(lo, hi)]  # noqa: E731
        out, share_at = [], 0
        for i in range(len(self)):
            segs = range(seg_off[i], seg_off[i + 1])
            n_sh = sum(en[g] - st[g] for g in segs)
            data = cut(sb, share_at, share_at + n_sh, SHARE_SIZE)
            share_at += n_sh
            if namespaces is None:
                if not self.one_namespace[i]:
                    parse_namespace(data, 0, len(data))
                ns = self.namespaces[i].tobytes()
            else:
                ns = bytes(namespaces[i])
            sp = [NMTProof(st[g], en[g], cut(nb, node_off[g], node_off[g + 1], NMT_ROOT_SIZE)) for g in segs]
            rp = [Proof(2 * W, idx[g], lb[32 * g:32 * (g + 1)], cut(ab, aunt_off[g], aunt_off[g + 1], 32))
                  for g in segs]
            out.append(ShareProof(data=data, share_proofs=sp, namespace_id=ns[1:],
                                  row_proof=RowProof(cut(rb, segs.start, segs.stop, NMT_ROOT_SIZE), rp, r0[i], r1[i]),
                                  namespace_version=ns[0]))
        return out


class SetShareProofs:
    """The share proofs of ranges across a ResidentSquareSet
    (cda_square_set_share_proofs): ONE flat ShareProofsBatch in request order
    and the square each range names."""

    def __init__(self, batch: ShareProofsBatch, squares):
        self.batch, self.squares = batch, np.ascontiguousarray(squares, dtype=np.uint32)

    def __len__(self):
        return len(self.batch)

    def data_roots(self, set_roots) -> np.ndarray:
        """One data root per proof, (n, 32), from the set's (n_squares, 32) data roots."""
        return np.ascontiguousarray(np.asarray(set_roots, dtype=np.uint8).reshape(-1, 32)[self.squares])

    def verify(self, data_roots, ctx=None) -> np.ndarray:
        """cda_share_proofs_verify of the batch, proof i against the data root
        of its square: data_roots is the set's (n_squares, 32) array
        (ResidentSquareSet.dah()[2]) or trusted roots of the same shape."""
        if len(self) == 0:
            return np.zeros(0, dtype=np.uint8)
        return self.batch.verify(self.data_roots(data_roots), ctx)

    def proofs(self, namespaces=None) -> list:
        """One ShareProof per range, as ShareProofsBatch.proofs."""
        return self.batch.proofs(namespaces)


# ------------------------------------------------- blob inclusion by share commitment
ERR_NOT_A_BLOB = "commitment proof is not one contiguous blob"
ERR_SUBTREE_ROOTS = "subtree roots failed to verify against the row roots"
ERR_COMMITMENT = "subtree roots do not hash to the share commitment"
# cda_commitment_proofs_verify's verdicts (include/cda.h); the numbering is this library's choice
COMMITMENT_VERDICT_TEXT = {0: None, 1: ERR_ROW_PROOF, 2: ERR_SUBTREE_ROOTS, 3: ERR_COMMITMENT, 4: ERR_NOT_A_BLOB}


def _u32_array(values, what: str) -> np.ndarray:
    a = np.asarray(values, dtype=np.int64).reshape(-1)
    if a.size and (a.min() < 0 or a.max() >= 1 << 32):
        raise _lib.CdaError(_lib.CDA_ERR_INVALID, f"{what} does not fit 32 bits")
    return np.ascontiguousarray(a.astype(np.uint32))


def commitment_proofs_plan(k: int, starts, share_lens, subtree_root_threshold: int = 64) -> dict:
    """cda_square_commitment_proofs_plan: n_segments, n_roots, n_nodes,
    n_aunts, aunts_per_segment of the batch of blobs (start, share_len) of a
    square of ODS width k.  Host only, no context; CdaError names the blob and
    the field."""
    st, ln = _u32_array(starts, "start"), _u32_array(share_lens, "share_len")
    if len(st) != len(ln):
        raise ValueError(f"{len(st)} starts but {len(ln)} share_lens")
    L = _lib.load()
    u32p = C.POINTER(C.c_uint32)
    p = _lib.CommitmentProofsPlanT()
    rc = L.cda_square_commitment_proofs_plan(k, st.ctypes.data_as(u32p), ln.ctypes.data_as(u32p), len(st),
                                             subtree_root_threshold, C.byref(p))
    if rc != _lib.CDA_OK:
        raise _lib.CdaError(rc, L.cda_last_error(None).decode())
    return {n: getattr(p, n) for n, _ in _lib.CommitmentProofsPlanT._fields_}


@dataclass
class CommitmentProof:              # celestia-node blob.CommitmentProof
    subtree_roots: list             # 90 bytes each, row by row, left to right
    subtree_root_proofs: list       # one NMTProof per row: the nodes of ProveRange(start, end)
    namespace: bytes                # 29 bytes
    row_proof: RowProof

    @property
    def share_len(self) -> int:
        """The blob's share count: the sum of the rows' ranges."""
        return sum(p.end - p.start for p in self.subtree_root_proofs)

    def validate(self, data_root: bytes, commitment: bytes, subtree_root_threshold: int = 64, ctx=None):
        """None when the blob with share commitment `commitment` lies in the
        square with `data_root`, else the verdict's text."""
        return validate_commitment_proofs([self], [data_root], [commitment], subtree_root_threshold, ctx)[0]


class CommitmentProofsBatch:
    """The commitment proofs of n blobs of one square as the flat arrays of
    cda_commitment_proofs_out (numpy; include/cda.h): proof i owns the
    segments (rows) seg_off[i] .. seg_off[i + 1], segment g the subtree roots
    root_off[g] .. root_off[g + 1], the nodes node_off[g] .. node_off[g + 1]
    and the aunts aunt_off[g] .. aunt_off[g + 1]."""

    FIELDS = tuple(n for n, _ in _lib.CommitmentProofsOut._fields_)

    def __init__(self, k, starts, share_lens, threshold, **arrays):
        self.k, self.starts, self.share_lens, self.threshold = k, starts, share_lens, threshold
        for name in self.FIELDS:
            setattr(self, name, arrays[name])

    @classmethod
    def empty(cls, k, starts, share_lens, threshold: int = 64, fill=None):
        """Buffers of the plan's sizes (filled with the byte `fill` if given)."""
        st, ln = _u32_array(starts, "start"), _u32_array(share_lens, "share_len")
        p = commitment_proofs_plan(k, st, ln, threshold)
        n, S = len(st), p["n_segments"]
        shapes = {"seg_off": ((n + 1,), np.uint32), "nmt_start": ((S,), np.int32), "nmt_end": ((S,), np.int32),
                  "node_off": ((S + 1,), np.uint32), "nodes": ((p["n_nodes"], NMT_ROOT_SIZE), np.uint8),
                  "row_roots": ((S, NMT_ROOT_SIZE), np.uint8), "rfc_total": ((S,), np.int64),
                  "rfc_index": ((S,), np.int64), "rfc_leaf_hash": ((S, 32), np.uint8),
                  "aunt_off": ((S + 1,), np.uint32), "aunts": ((p["n_aunts"], 32), np.uint8),
                  "namespaces": ((n, 29), np.uint8), "start_row": ((n,), np.uint32), "end_row": ((n,), np.uint32),
                  "root_off": ((S + 1,), np.uint32), "subtree_roots": ((p["n_roots"], NMT_ROOT_SIZE), np.uint8),
                  "norm_start": ((n,), np.uint32), "commitments": ((n, 32), np.uint8)}
        arrays = {}
        for name, (shape, dtype) in shapes.items():
            a = np.empty(shape, dtype=dtype)
            if fill is not None:
                a.view(np.uint8).fill(fill)
            arrays[name] = a
        return cls(k, st, ln, threshold, **arrays)

    def __len__(self):
        return len(self.starts)

    def arrays(self):
        return tuple(getattr(self, name) for name in self.FIELDS)

    def out_struct(self, skip=()):
        """cda_commitment_proofs_out over the arrays (NULL for the names in `skip`)."""
        o = _lib.CommitmentProofsOut()
        for (name, t), a in zip(_lib.CommitmentProofsOut._fields_, self.arrays()):
            if name not in skip:
                setattr(o, name, a.ctypes.data_as(t))
        return o

    def batch(self, data_root, commitments=None):
        """The cda_commitment_proof_batch over these arrays, unchanged: pointer
        assignment.  data_root: 32 bytes for every proof, or n * 32;
        commitments: n * 32 claimed commitments (None: the batch's own)."""
        n = len(self)
        roots = np.frombuffer(bytes(data_root), dtype=np.uint8) if isinstance(data_root, (bytes, bytearray)) \
            else np.ascontiguousarray(data_root, dtype=np.uint8).reshape(-1)
        if roots.size == 32:
            roots = np.tile(roots, max(1, n))
        if roots.size != 32 * max(1, n):
            raise ValueError(f"{n} proofs but {roots.size} bytes of data roots")
        if commitments is None:
            claimed = self.commitments.reshape(-1)
        else:
            claimed = np.frombuffer(b"".join(bytes(c) for c in commitments), dtype=np.uint8)
        if claimed.size != 32 * n:
            raise ValueError(f"{n} proofs but {claimed.size} bytes of commitments")
        if not claimed.size:
            claimed = np.zeros(32, dtype=np.uint8)
        b = _lib.CommitmentProofBatch()
        b.n_proofs, b.ns_len, b.threshold = n, 29, self.threshold
        b.data_roots = roots.ctypes.data_as(_lib.CommitmentProofBatch._u8p)
        b.commitments = claimed.ctypes.data_as(_lib.CommitmentProofBatch._u8p)
        for name, t in _lib.CommitmentProofBatch._fields_:
            if name in self.FIELDS and name != "commitments":
                setattr(b, name, getattr(self, name).ctypes.data_as(t))
        b.n_nodes, b.n_roots, b.n_aunts = len(self.nodes), len(self.subtree_roots), len(self.aunts)
        b._keep = (roots, claimed, self)   # the struct borrows the arrays
        return b

    def verify(self, data_root, commitments=None, ctx=None) -> np.ndarray:
        """cda_commitment_proofs_verify of the batch: the verdict per proof
        (COMMITMENT_VERDICT_TEXT)."""
        ctx = ctx or default_context()
        b = self.batch(data_root, commitments)
        verdict = np.full(max(1, len(self)), 255, dtype=np.uint8)
        ctx.check(ctx.lib.cda_commitment_proofs_verify(ctx.h, C.byref(b), ptr(verdict)))
        return verdict[:len(self)]

    def proofs(self) -> list:
        """One CommitmentProof per blob."""
        W = 2 * self.k
        nb, rb, lb, ab, sb = (a.tobytes() for a in (self.nodes, self.row_roots, self.rfc_leaf_hash, self.aunts,
                                                    self.subtree_roots))
        seg_off, node_off, aunt_off = self.seg_off.tolist(), self.node_off.tolist(), self.aunt_off.tolist()
        root_off = self.root_off.tolist()
        st, en, idx = self.nmt_start.tolist(), self.nmt_end.tolist(), self.rfc_index.tolist()
        r0, r1 = self.start_row.tolist(), self.end_row.tolist()
        cut = lambda b, lo, hi, sz: [b[i * sz:(i + 1) * sz] for i in range(lo, hi)]  # noqa: E731
        out = []
        for i in range(len(self)):
            segs = range(seg_off[i], seg_off[i + 1])
            sp = [NMTProof(st[g], en[g], cut(nb, node_off[g], node_off[g + 1], NMT_ROOT_SIZE)) for g in segs]
            rp = [Proof(2 * W, idx[g], lb[32 * g:32 * (g + 1)], cut(ab, aunt_off[g], aunt_off[g + 1], 32))
                  for g in segs]
            out.append(CommitmentProof(
                subtree_roots=cut(sb, root_off[segs.start], root_off[segs.stop], NMT_ROOT_SIZE),
                subtree_root_proofs=sp, namespace=self.namespaces[i].tobytes(),
                row_proof=RowProof(cut(rb, segs.start, segs.stop, NMT_ROOT_SIZE), rp, r0[i], r1[i])))
        return out


def build_commitment_proof_batch(proofs, data_roots, commitments, subtree_root_threshold: int = 64,
                                 roots_per_row=None):
    """The cda_commitment_proof_batch of CommitmentProof objects (any mix of
    square widths) and the arrays it points into.  A proof's subtree roots are
    dealt to its rows by the cover's counts for the rows' ranges and the
    threshold -- the last row takes what remains, so a proof with too many or
    too few roots fails there; roots_per_row (one list of counts per proof)
    overrides that split."""
    from . import inclusion
    u8p, u32p, i32p, i64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_int32, C.c_int64))
    keep = []

    def arr(a, t):
        keep.append(a)
        return a.ctypes.data_as(t)

    def offsets(counts):
        return np.cumsum([0] + list(counts), dtype=np.int64).astype(np.uint32)

    segs, root_counts = [], []
    for i, p in enumerate(proofs):
        rows = list(zip(p.subtree_root_proofs, p.row_proof.row_roots, p.row_proof.proofs))
        if roots_per_row is not None and roots_per_row[i] is not None:
            counts = list(roots_per_row[i])
        else:
            n_sh = sum(max(0, q.end - q.start) for q, _, _ in rows)
            w = inclusion.sub_tree_width(n_sh, subtree_root_threshold) if n_sh else 1
            counts, left = [], len(p.subtree_roots)
            for j, (q, _, _) in enumerate(rows):
                c = _cover_count(q.start, q.end, w) if j + 1 < len(rows) else left
                c = min(c, left)
                counts.append(c)
                left -= c
        segs += rows
        root_counts += counts
    b = _lib.CommitmentProofBatch()
    b.n_proofs, b.ns_len, b.threshold = len(proofs), 29, subtree_root_threshold
    b.data_roots = arr(_bytes_array(data_roots), u8p)
    b.commitments = arr(_bytes_array(commitments), u8p)
    b.seg_off = arr(offsets(len(p.subtree_root_proofs) for p in proofs), u32p)
    b.nmt_start = arr(np.array([q.start for q, _, _ in segs] or [0], dtype=np.int32), i32p)
    b.nmt_end = arr(np.array([q.end for q, _, _ in segs] or [0], dtype=np.int32), i32p)
    b.node_off = arr(offsets(len(q.nodes) for q, _, _ in segs), u32p)
    b.nodes = arr(_bytes_array(x for q, _, _ in segs for x in q.nodes), u8p)
    b.n_nodes = sum(len(q.nodes) for q, _, _ in segs)
    b.root_off = arr(offsets(root_counts), u32p)
    b.subtree_roots = arr(_bytes_array(x for p in proofs for x in p.subtree_roots), u8p)
    b.n_roots = sum(len(p.subtree_roots) for p in proofs)
    b.row_roots = arr(_bytes_array(r for _, r, _ in segs), u8p)
    b.rfc_total = arr(np.array([m.total for _, _, m in segs] or [0], dtype=np.int64), i64p)
    b.rfc_index = arr(np.array([m.index for _, _, m in segs] or [0], dtype=np.int64), i64p)
    b.rfc_leaf_hash = arr(_bytes_array(m.leaf_hash for _, _, m in segs), u8p)
    b.aunt_off = arr(offsets(len(m.aunts) for _, _, m in segs), u32p)
    b.aunts = arr(_bytes_array(a for _, _, m in segs for a in m.aunts), u8p)
    b.n_aunts = sum(len(m.aunts) for _, _, m in segs)
    return b, keep


def _cover_count(s0: int, e0: int, w: int) -> int:
    """The number of subtree roots of the leaf range [s0, e0) with width w
    (csrc/commitment_proofs_plan.h subtree_cover_count)."""
    n, c = 0, s0
    while c < e0:
        r = w
        while c % r or c + r > e0:
            r //= 2
        n, c = n + 1, c + r
    return n


def _commitment_proof_well_formed(p, data_root, commitment) -> bool:
    """A proof the batch call can carry: 90-byte nodes and roots, 32-byte
    hashes, int32 ranges within the library's bound, as many row roots and
    merkle proofs as NMT proofs."""
    rp = p.row_proof
    return len(data_root) == 32 and len(commitment) == 32 and len(p.namespace) == 29 and \
        len(p.subtree_root_proofs) == len(rp.row_roots) == len(rp.proofs) and \
        all(len(r) == NMT_ROOT_SIZE for r in p.subtree_roots) and all(len(r) == NMT_ROOT_SIZE for r in rp.row_roots) and \
        all(len(x) == NMT_ROOT_SIZE for q in p.subtree_root_proofs for x in q.nodes) and \
        all(0 <= q.start < q.end <= _lib.VERIFY_MAX_LEAVES for q in p.subtree_root_proofs) and \
        all(_proof_well_formed(m) for m in rp.proofs)


def validate_commitment_proofs(proofs, data_roots, commitments, subtree_root_threshold: int = 64, ctx=None) -> list:
    """CommitmentProof.validate for many proofs, from squares of any width, in
    one cda_commitment_proofs_verify call: per proof None or the verdict's
    text.  A proof with a field of the wrong length, or without a row, cannot
    be one blob's and is answered ERR_NOT_A_BLOB without reaching the GPU."""
    if not len(proofs) == len(data_roots) == len(commitments):
        raise ValueError(f"{len(proofs)} proofs, {len(data_roots)} data roots, {len(commitments)} commitments")
    out = [ERR_NOT_A_BLOB] * len(proofs)
    idx = [i for i, p in enumerate(proofs) if _commitment_proof_well_formed(p, data_roots[i], commitments[i])]
    if idx:
        ctx = ctx or default_context()
        b, keep = build_commitment_proof_batch([proofs[i] for i in idx], [bytes(data_roots[i]) for i in idx],
                                               [bytes(commitments[i]) for i in idx], subtree_root_threshold)
        verdict = np.full(len(idx), 255, dtype=np.uint8)
        ctx.check(ctx.lib.cda_commitment_proofs_verify(ctx.h, C.byref(b), ptr(verdict)))
        del keep
        for i, v in zip(idx, verdict.tolist()):
            out[i] = COMMITMENT_VERDICT_TEXT[v]
    return out


# ------------------------------------------------------------ verification
def _proof_well_formed(q) -> bool:
    """A merkle Proof the batch call can carry: 32-byte hashes, int64 fields.
    Anything else cannot verify (the hashes would differ in length)."""
    return len(q.leaf_hash) == 32 and all(len(a) == 32 for a in q.aunts) and \
        -(1 << 63) <= q.total < (1 << 63) and -(1 << 63) <= q.index < (1 << 63)


def _row_well_formed(sp, root) -> bool:
    n = 2 * (1 + len(sp.namespace_id)) + 32
    return len(root) == 32 and all(len(r) == n for r in sp.row_proof.row_roots) and \
        all(_proof_well_formed(q) for q in sp.row_proof.proofs)


def _nmt_well_formed(sp) -> bool:
    """The NMT half fits the batch layout: a one-byte namespace version, nodes
    of 2*ns_len + 32 bytes, shares of one length.  Anything else fails
    VerifyProof in the reference too.  (A namespace longer than the library's
    bound is the call's CDA_ERR_INVALID, not a verdict.)"""
    n = 2 * (1 + len(sp.namespace_id)) + 32
    return 0 <= sp.namespace_version <= 255 and \
        all(len(x) == n for p in sp.share_proofs for x in p.nodes) and \
        all(len(r) == n for r in sp.row_proof.row_roots) and len({len(s) for s in sp.data}) == 1


def _bytes_array(parts) -> np.ndarray:
    a = np.frombuffer(b"".join(bytes(p) for p in parts), dtype=np.uint8)
    return a if a.size else np.zeros(1, dtype=np.uint8)


def _build_batch(ns_len: int, share_len: int, entries, rows: bool, nmt: bool):
    """The cda_share_proof_batch of `entries`: (namespace, data root or None,
    segments, shares) per proof, segments: (start, end, nodes, row root,
    merkle Proof or None) per row.  Returns (struct, arrays it points into)."""
    segs = [s for e in entries for s in e[2]]
    u8p, u32p, i32p, i64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_int32, C.c_int64))
    keep = []

    def arr(a, t):
        keep.append(a)
        return a.ctypes.data_as(t)

    def offsets(counts):
        return np.cumsum([0] + list(counts), dtype=np.int64).astype(np.uint32)

    b = _lib.ShareProofBatch()
    b.n_proofs, b.ns_len, b.share_len = len(entries), ns_len, share_len
    b.namespaces = arr(_bytes_array(e[0] for e in entries), u8p)
    b.seg_off = arr(offsets(len(e[2]) for e in entries), u32p)
    b.row_roots = arr(_bytes_array(s[3] for s in segs), u8p)
    if rows:
        b.data_roots = arr(_bytes_array(e[1] for e in entries), u8p)
        b.rfc_total = arr(np.array([s[4].total for s in segs] or [0], dtype=np.int64), i64p)
        b.rfc_index = arr(np.array([s[4].index for s in segs] or [0], dtype=np.int64), i64p)
        b.rfc_leaf_hash = arr(_bytes_array(s[4].leaf_hash for s in segs), u8p)
        b.aunt_off = arr(offsets(len(s[4].aunts) for s in segs), u32p)
        b.aunts = arr(_bytes_array(a for s in segs for a in s[4].aunts), u8p)
        b.n_aunts = sum(len(s[4].aunts) for s in segs)
    if nmt:
        b.nmt_start = arr(np.array([s[0] for s in segs] or [0], dtype=np.int32), i32p)
        b.nmt_end = arr(np.array([s[1] for s in segs] or [0], dtype=np.int32), i32p)
        b.node_off = arr(offsets(len(s[2]) for s in segs), u32p)
        b.nodes = arr(_bytes_array(x for s in segs for x in s[2]), u8p)
        b.n_nodes = sum(len(s[2]) for s in segs)
        b.shares = arr(_bytes_array(x for e in entries for x in e[3]), u8p)
        b.n_shares = sum(len(e[3]) for e in entries)
    return b, keep


def _verify_batch(ctx, ns_len: int, share_len: int, entries, rows: bool, nmt: bool) -> list:
    """One cda_share_proofs_verify call over `entries` (_build_batch): the
    verdict per proof (0 valid, 1 row proof, 2 share proof)."""
    ctx = ctx or default_context()
    b, keep = _build_batch(ns_len, share_len, entries, rows, nmt)
    verdict = np.full(max(1, len(entries)), 255, dtype=np.uint8)
    ctx.check(ctx.lib.cda_share_proofs_verify(ctx.h, C.byref(b), ptr(verdict)))
    del keep
    return [int(v) for v in verdict[:len(entries)]]


def validate_share_proofs(proofs, roots, ctx=None) -> list:
    """ShareProof.Validate(root) for many proofs at once: per proof None, or
    the reference's error text.  Proofs that fail a structural check are
    answered here and never reach the GPU; the rest go into one
    cda_share_proofs_verify call per distinct namespace length (and share
    length).  A field of the wrong length cannot verify in the reference
    either (its hash, or the comparison, differs), so such a proof gets the
    verdict Validate gives without being hashed: a malformed row root, leaf
    hash, aunt or data root is "row proof failed to verify"; a malformed NMT
    node, share or namespace version is "share proof failed to verify", and
    only if the proof's row proofs verify (they run in a row-only call)."""
    if len(proofs) != len(roots):
        raise ValueError(f"{len(proofs)} proofs but {len(roots)} roots")
    out = [None] * len(proofs)
    full, row_only = {}, {}   # (ns_len, share_len) -> proof indexes
    for i, (p, root) in enumerate(zip(proofs, roots)):
        err = p.structural_error()
        if err is not None:
            out[i] = err
        elif not _row_well_formed(p, root):
            out[i] = ERR_ROW_PROOF
        elif not _nmt_well_formed(p):
            row_only.setdefault((1 + len(p.namespace_id), 0), []).append(i)
        else:
            full.setdefault((1 + len(p.namespace_id), len(p.data[0])), []).append(i)
    for groups, nmt in ((full, True), (row_only, False)):
        for (ns_len, share_len), idx in groups.items():
            entries = []
            for i in idx:
                p = proofs[i]
                ns = bytes([p.namespace_version & 0xFF]) + bytes(p.namespace_id)
                segs = [(s.start, s.end, s.nodes if nmt else [], r, q)
                        for s, r, q in zip(p.share_proofs, p.row_proof.row_roots, p.row_proof.proofs)]
                entries.append((ns, bytes(roots[i]), segs, p.data if nmt else []))
            for i, v in zip(idx, _verify_batch(ctx, ns_len, share_len, entries, rows=True, nmt=nmt)):
                out[i] = ERR_ROW_PROOF if v == 1 else ERR_SHARE_PROOF if (v == 2 or not nmt) else None
    return out


def nmt_verify_inclusion(root: bytes, nodes, start: int, end: int, namespace: bytes, leaves, ctx=None) -> bool:
    """nmt Proof.VerifyInclusion (IgnoreMaxNamespace proofs) of `leaves` as
    leaves [start, end) under `namespace` (version || id) against `root`: the
    NMT half of VerifyProof alone, pairing with cda_nmt_prove_range and
    wrapper's ProveRange."""
    n = 2 * len(namespace) + 32
    leaves = [bytes(x) for x in leaves]
    if start < 0 or end <= start or len(leaves) != end - start or len(root) != n or \
            any(len(x) != n for x in nodes) or len({len(x) for x in leaves}) != 1:
        return False
    seg = (start, end, [bytes(x) for x in nodes], bytes(root), None)
    return _verify_batch(ctx, len(namespace), len(leaves[0]), [(bytes(namespace), None, [seg], leaves)],
                         rows=False, nmt=True)[0] == 0


def _go_namespace(ns: bytes) -> str:
    """fmt %v of a go-square namespace.Namespace{Version, ID}."""
    return "{%d [%s]}" % (ns[0], " ".join(str(b) for b in ns[1:]))


def parse_namespace(raw_shares, start_share: int, end_share: int) -> bytes:
    """proof.ParseNamespace (pkg/proof/querier.go:134-166): the one namespace
    (29 bytes) of shares [start_share, end_share), with the reference's
    error texts (ValueError)."""
    if start_share < 0:
        raise ValueError(f"start share {start_share} should be positive")
    if end_share < 0:
        raise ValueError(f"end share {end_share} should be positive")
    if end_share <= start_share:
        raise ValueError(f"end share {end_share} cannot be lower or equal to the starting share {start_share}")
    if end_share > len(raw_shares):
        raise ValueError(f"end share {end_share} is higher than block shares {len(raw_shares)}")
    first = bytes(raw_shares[start_share][:29])
    for i, sh in enumerate(raw_shares[start_share:end_share]):
        ns = bytes(sh[:29])
        if ns != first:
            raise ValueError(f"shares range contain different namespaces at index {i}: "
                             f"{_go_namespace(first)} and {_go_namespace(ns)} ")
    return first


TX_NAMESPACE = b"\x00" * 28 + b"\x01"            # go-square namespace.TxNamespace
PAY_FOR_BLOB_NAMESPACE = b"\x00" * 28 + b"\x04"  # namespace.PayForBlobNamespace


def tx_share_range(txs, tx_index: int, max_square_size: int = 128, subtree_root_threshold: int = 64):
    """builder.FindTxShareRange of square.Construct's layout: (start, end,
    namespace) -- the tx namespace for a normal tx, the PFB namespace for a
    blob tx (proof.go:51-57 getTxNamespace).  Host only."""
    from .square import _flatten, _u64p
    L = _lib.load()
    buf, off = _flatten(txs)
    s, e, pfb = C.c_uint32(), C.c_uint32(), C.c_int()
    rc = L.cda_square_tx_share_range(None, ptr(buf), _u64p(off), len(txs), max_square_size, subtree_root_threshold,
                                     tx_index, C.byref(s), C.byref(e), C.byref(pfb))
    if rc != _lib.CDA_OK:
        msg = L.cda_last_error(None).decode()
        raise (_lib.SquareError if rc == _lib.CDA_ERR_SQUARE else _lib.CdaError)(rc, msg)
    return s.value, e.value, PAY_FOR_BLOB_NAMESPACE if pfb.value else TX_NAMESPACE


def tx_share_ranges(txs, tx_indexes, max_square_size: int = 128, subtree_root_threshold: int = 64) -> list:
    """tx_share_range for every index of tx_indexes, with the square laid out
    once (cda_square_tx_share_ranges): a list of (start, end, namespace).
    Host only."""
    from .square import _flatten, _u64p
    L = _lib.load()
    buf, off = _flatten(txs)
    idx = np.ascontiguousarray(tx_indexes, dtype=np.uint32)
    n = idx.size
    s, e, pfb = np.empty(max(1, n), dtype=np.uint32), np.empty(max(1, n), dtype=np.uint32), \
        np.empty(max(1, n), dtype=np.uint8)
    u32p = C.POINTER(C.c_uint32)
    rc = L.cda_square_tx_share_ranges(None, ptr(buf), _u64p(off), len(txs), max_square_size, subtree_root_threshold,
                                      idx.ctypes.data_as(u32p), n, s.ctypes.data_as(u32p), e.ctypes.data_as(u32p),
                                      ptr(pfb))
    if rc != _lib.CDA_OK:
        msg = L.cda_last_error(None).decode()
        raise (_lib.SquareError if rc == _lib.CDA_ERR_SQUARE else _lib.CdaError)(rc, msg)
    return [(int(s[i]), int(e[i]), PAY_FOR_BLOB_NAMESPACE if pfb[i] else TX_NAMESPACE) for i in range(n)]


def new_share_inclusion_proof(ods, namespace: bytes, start: int, end: int, ctx=None) -> ShareProof:
    """NewShareInclusionProof (proof.go:59-73): extend the square, prove the
    range.  ods: the square's shares (bytes, a list of shares or an array)."""
    if isinstance(ods, (bytes, bytearray, memoryview)):
        ods = np.frombuffer(ods, dtype=np.uint8)
    elif isinstance(ods, list):
        ods = np.frombuffer(b"".join(ods), dtype=np.uint8)
    sq = ResidentSquare(ods, ctx)
    try:
        return sq.share_proof(namespace, start, end)
    finally:
        sq.close()


def new_tx_inclusion_proof(txs, tx_index: int, app_version: int = 2, ctx=None) -> ShareProof:
    """NewTxInclusionProof (proof.go:22-49): the share proof of the shares that
    hold tx tx_index of the block, in the square square.Construct builds."""
    from . import square
    if tx_index < 0:   # the Go parameter is a uint64
        raise _lib.CdaError(_lib.CDA_ERR_INVALID, f"txIndex {tx_index} is negative")
    if tx_index >= len(txs):
        raise _lib.CdaError(_lib.CDA_ERR_INVALID, f"txIndex {tx_index} out of bounds")
    ub, thr = square.SQUARE_SIZE_UPPER_BOUND, square.SUBTREE_ROOT_THRESHOLD   # appconsts, every version
    start, end, ns = tx_share_range(txs, tx_index, ub, thr)
    sq = square.construct(txs, ub, thr, ctx=ctx)
    return new_share_inclusion_proof(sq.to_bytes(), ns, start, end, ctx)


def new_share_inclusion_proofs(ods, ranges, namespaces=None, ctx=None) -> list:
    """NewShareInclusionProof for every (start, end) of `ranges` over one
    square: one extension and one batch call (ResidentSquare.
    share_proofs_batch).  namespaces: as ShareProofsBatch.proofs."""
    if isinstance(ods, (bytes, bytearray, memoryview)):
        ods = np.frombuffer(ods, dtype=np.uint8)
    elif isinstance(ods, list):
        ods = np.frombuffer(b"".join(ods), dtype=np.uint8)
    sq = ResidentSquare(ods, ctx)
    try:
        return sq.share_proofs_batch(ranges).proofs(namespaces)
    finally:
        sq.close()


def new_tx_inclusion_proofs(txs, indexes=None, app_version: int = 2, ctx=None) -> list:
    """NewTxInclusionProof for the transactions `indexes` of a block (None:
    every transaction): one square.Construct, one resident square and one
    batch call; equal to [new_tx_inclusion_proof(txs, i) for i in indexes]."""
    from . import square
    indexes = list(range(len(txs))) if indexes is None else [int(i) for i in indexes]
    for i in indexes:
        if i < 0:   # the Go parameter is a uint64
            raise _lib.CdaError(_lib.CDA_ERR_INVALID, f"txIndex {i} is negative")
        if i >= len(txs):
            raise _lib.CdaError(_lib.CDA_ERR_INVALID, f"txIndex {i} out of bounds")
    if not indexes:
        return []
    ub, thr = square.SQUARE_SIZE_UPPER_BOUND, square.SUBTREE_ROOT_THRESHOLD   # appconsts, every version
    found = tx_share_ranges(txs, indexes, ub, thr)
    sq = square.construct(txs, ub, thr, ctx=ctx)
    return new_share_inclusion_proofs(sq.to_bytes(), [(s, e) for s, e, _ in found], [ns for _, _, ns in found], ctx)


def _parse_int64(text: str) -> int:
    """strconv.ParseInt(text, 10, 64) with Go's error texts (ValueError)."""
    if not text or text.strip() != text or "_" in text:   # Go's base-10 syntax
        raise ValueError(f'strconv.ParseInt: parsing "{text}": invalid syntax')
    try:
        v = int(text, 10)
    except ValueError:
        raise ValueError(f'strconv.ParseInt: parsing "{text}": invalid syntax') from None
    if not -(1 << 63) <= v < (1 << 63):
        raise ValueError(f'strconv.ParseInt: parsing "{text}": value out of range')
    return v


def query_tx_inclusion_proof(path, txs, app_version: int = 2, ctx=None) -> ShareProof:
    """QueryTxInclusionProof's index handling (pkg/proof/querier.go:29-57) over
    a block's txs (the ABCI query's protobuf block is the caller's): path is
    the query path, [index]; errors are ValueError with the reference texts."""
    if len(path) != 1:
        raise ValueError(f"expected query path length: 1 actual: {len(path)} ")
    index = _parse_int64(path[0])
    if index < 0:
        raise ValueError(f'path[0] element: "{path[0]}" produced a negative value: {index}')
    return new_tx_inclusion_proof(txs, index, app_version, ctx)


def query_share_inclusion_proof(path, txs, app_version: int = 2, ctx=None) -> ShareProof:
    """QueryShareInclusionProof (pkg/proof/querier.go:72-128): path = [begin,
    end]; the block's square is square.Construct at the version's upper bound,
    the range must hold one namespace (ParseNamespace), then
    NewShareInclusionProof on the GPU."""
    from . import square
    if len(path) != 2:
        raise ValueError(f"expected query path length: 2 actual: {len(path)} ")
    begin, end = _parse_int64(path[0]), _parse_int64(path[1])
    sq = square.construct(txs, square.SQUARE_SIZE_UPPER_BOUND, square.SUBTREE_ROOT_THRESHOLD, ctx=ctx)
    ns = parse_namespace(sq, begin, end)
    return new_share_inclusion_proof(sq.to_bytes(), ns, begin, end, ctx)


def _pb_fields(buf: bytes):
    """(field number, wire type, value) of a protobuf message; ValueError if it
    does not parse."""
    i, n = 0, len(buf)

    def varint():
        nonlocal i
        v = shift = 0
        while True:
            if i >= n or shift > 63:
                raise ValueError("malformed varint")
            c = buf[i]
            i += 1
            v |= (c & 0x7F) << shift
            shift += 7
            if c < 0x80:
                return v

    while i < n:
        key = varint()
        fn, wt = key >> 3, key & 7
        if wt == 0:
            yield fn, wt, varint()
        elif wt == 2:
            ln = varint()
            if i + ln > n:
                raise ValueError("field beyond the message")
            yield fn, wt, buf[i:i + ln]
            i += ln
        elif wt in (1, 5):
            ln = 8 if wt == 1 else 4
            if i + ln > n:
                raise ValueError("field beyond the message")
            yield fn, wt, buf[i:i + ln]
            i += ln
        else:
            raise ValueError(f"wire type {wt}")


def blob_tx_blobs(tx: bytes):
    """The blobs of a BlobTx and what its MsgPayForBlobs commits to: a list of
    (share count, share commitment or None) in the tx's order, or None if tx
    is not a BlobTx (go-square blob.UnmarshalBlobTx: type_id "BLOB")."""
    from . import inclusion
    try:
        top = list(_pb_fields(tx))
        if not any(fn == 3 and wt == 2 and v == b"BLOB" for fn, wt, v in top):
            return None
        inner = b"".join(v for fn, wt, v in top if fn == 1 and wt == 2)
        sizes = []
        for fn, wt, v in top:
            if fn == 2 and wt == 2:
                sizes.append(sum(len(d) for f, w, d in _pb_fields(v) if f == 2 and w == 2))
    except ValueError:
        return None
    commits = pfb_share_commitments(inner)
    return [(inclusion.sparse_shares_needed(sz), commits[i] if i < len(commits) else None)
            for i, sz in enumerate(sizes)]


def pfb_share_commitments(inner: bytes) -> list:
    """The share commitments of the MsgPayForBlobs in the signed tx `inner` (a
    BlobTx's tx, an IndexWrapper's tx); [] when it does not decode."""
    try:   # TxRaw.body_bytes -> TxBody.messages -> Any{type_url, value} -> MsgPayForBlobs.share_commitments
        body = b"".join(v for fn, wt, v in _pb_fields(inner) if fn == 1 and wt == 2)
        for fn, wt, v in _pb_fields(body):
            if fn != 1 or wt != 2:
                continue
            msg = {f: d for f, w, d in _pb_fields(v) if w == 2}
            if msg.get(1) == b"/celestia.blob.v1.MsgPayForBlobs":
                return [d for f, w, d in _pb_fields(msg.get(2, b"")) if f == 4 and w == 2]
    except ValueError:
        pass
    return []


def new_blob_commitment_proofs(txs, app_version: int = 2, ctx=None) -> list:
    """The commitment proof of every blob of a block, in PFB order (blob txs in
    block order, a tx's blobs in its order): a list of (CommitmentProof,
    claimed share commitment or None when the PFB does not decode).  The blob
    starts are square.Construct's share indexes, the lengths the blobs', the
    commitments the PFBs'; one square.Construct, one resident square, one
    cda_square_commitment_proofs call."""
    from . import square
    ub, thr = square.SQUARE_SIZE_UPPER_BOUND, square.SUBTREE_ROOT_THRESHOLD   # appconsts, every version
    blobs = [b for tx in txs for b in (blob_tx_blobs(tx) or [])]
    if not blobs:
        return []
    _, _, share_indexes = square.layout(txs, ub, thr)
    if len(share_indexes) != len(blobs):
        raise _lib.CdaError(_lib.CDA_ERR_INVALID, f"the layout places {len(share_indexes)} blobs, the txs hold {len(blobs)}")
    sq = ResidentSquare(np.frombuffer(square.construct(txs, ub, thr, ctx=ctx).to_bytes(), dtype=np.uint8), ctx)
    try:
        batch = sq.commitment_proofs(share_indexes, [n for n, _ in blobs], thr)
    finally:
        sq.close()
    return list(zip(batch.proofs(), [c for _, c in blobs]))


def new_blob_commitment_proofs_from_square(sq: ResidentSquare, subtree_root_threshold: int = 64) -> list:
    """new_blob_commitment_proofs for a node that holds only the square (an EDS it
    received, or one repaired from samples): the blobs' starts and lengths come
    from ResidentSquare.parse (the table only, no blob bytes), the claimed
    commitments from the MsgPayForBlobs inside the PFBs' IndexWrappers, the
    order is the PFBs' (a PFB's blobs by its share_indexes).  One parse, one
    cda_square_commitment_proofs call on the same resident square."""
    from . import shares
    parsed = sq.parse(blob_data=False)
    share_len = dict(zip(parsed.blob_starts, parsed.blob_share_lens))
    starts, lens, claimed = [], [], []
    for unit in parsed.pfbs:
        inner, idx = shares.unmarshal_index_wrapper(unit)
        commits = pfb_share_commitments(inner)
        for i, start in enumerate(idx):
            if start not in share_len:
                raise _lib.CdaError(_lib.CDA_ERR_INVALID, f"a PFB names share {start}, where no blob starts")
            starts.append(start)
            lens.append(share_len[start])
            claimed.append(commits[i] if i < len(commits) else None)
    if not starts:
        return []
    batch = sq.commitment_proofs(starts, lens, subtree_root_threshold)
    return list(zip(batch.proofs(), claimed))

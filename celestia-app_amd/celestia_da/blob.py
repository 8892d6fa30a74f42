"""Blobs of a resident square by namespace and by share commitment: what a user
of a data-availability layer asks a node most.

The model is celestia-node's blob.Service.GetAll(height, namespaces) and
blob.Service.Get(height, namespace, commitment), restated from their published
behaviour and unpinned (no vector of theirs is here): GetAll returns every blob
of the namespaces, Get the blob of a namespace whose share commitment is the
given one.  The node holds only the square; nothing here reads the block's txs.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .namespace import INCLUSION, NamespaceProofsBatch, _namespaces_array, namespace_plan


class BlobNotFoundError(LookupError):
    """blob.ErrBlobNotFound: no blob of the namespace has the commitment."""


def namespace_ranges(sq, namespaces) -> list:
    """The share ranges [(start, end)] of the original square that hold the
    shares of `namespaces` (29 bytes each), ascending and disjoint, runs that
    continue over a row's end merged: cda_square_namespace_proofs with the
    share, node and leaf buffers NULL gives row and leaf range of every run."""
    ns = np.unique(_namespaces_array(namespaces), axis=0)
    if len(ns) == 0:
        return []
    batch = NamespaceProofsBatch.empty(sq.k, ns, namespace_plan(sq, ns))
    o = batch.out_struct(skip=("nodes", "shares", "absence_leaf"))
    sq.ctx.check(sq.ctx.lib.cda_square_namespace_proofs(sq.h, _lib.ptr(batch.namespaces), len(ns), o))
    runs = sorted((int(r) * sq.k + int(s), int(r) * sq.k + int(e))
                  for r, kind, s, e in zip(batch.row, batch.kind, batch.nmt_start, batch.nmt_end) if kind == INCLUSION)
    merged = []
    for s, e in runs:
        if merged and merged[-1][1] == s:
            merged[-1][1] = e
        else:
            merged.append([s, e])
    return [tuple(x) for x in merged]


def get_all(sq, namespaces) -> list:
    """blob.Service.GetAll: every blob of `namespaces` in the resident square
    `sq`, as inclusion.Blob in square order.  One namespace search for the
    ranges, one parse call for all of them."""
    ranges = namespace_ranges(sq, namespaces)
    return sq.parse(ranges).blobs if ranges else []


def get(sq, namespace: bytes, commitment: bytes, threshold: int = 64):
    """blob.Service.Get: the blob of `namespace` whose share commitment is
    `commitment`.  The namespace's ranges are parsed for their table only, the
    commitments of its blobs come from the square's cached row trees
    (ResidentSquare.blob_commitments), and only the match's bytes are gathered.
    BlobNotFoundError if there is none."""
    ranges = namespace_ranges(sq, [namespace])
    table = sq.parse(ranges, blob_data=False) if ranges else None
    if table is not None and table.blob_starts:
        commitments = sq.blob_commitments(table.blob_starts, table.blob_share_lens, threshold)
        for start, n, c in zip(table.blob_starts, table.blob_share_lens, commitments):
            if c == bytes(commitment):
                return sq.parse([(start, start + n)]).blobs[0]
    raise BlobNotFoundError(f"no blob of namespace {bytes(namespace).hex()} has commitment {bytes(commitment).hex()}")

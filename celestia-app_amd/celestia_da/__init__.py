"""celestia_da -- MI355X-native celestia-app data-availability hot path.

Host-side mirror of the reference's Go API (pkg/da, pkg/wrapper, rsmt2d,
go-square square) over the C ABI of libcda.so (include/cda.h).  See DESIGN.md.
"""
from . import (_lib, app, axis_halves, blob, blobfactory, byzantine, da, inclusion, malicious, namespace, proof, replay, rsmt2d, sampling, shares, square,  # noqa: F401
               wrapper)
from .namespace import (get_shares_by_namespace, get_shares_by_namespace_set, verify_namespaced_shares,  # noqa: F401
                        verify_namespaced_shares_set)
from ._lib import (ByzantineDataError, CdaError, Context, PushOrderError, SquareError, UnrepairableError,  # noqa: F401
                   default_context, load)

__all__ = ["app", "da", "rsmt2d", "wrapper", "square", "inclusion", "proof", "namespace", "sampling", "axis_halves", "replay", "malicious", "blobfactory", "byzantine", "shares", "blob", "Context", "CdaError", "PushOrderError", "SquareError",
           "ByzantineDataError", "UnrepairableError",
           "default_context", "load", "get_shares_by_namespace", "verify_namespaced_shares",
           "get_shares_by_namespace_set", "verify_namespaced_shares_set"]

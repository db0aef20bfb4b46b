"""MI355X-native per-inverted-list ID codecs (ROC / bits-back ANS, Elias-Fano, packed bits).

Hot path of facebookresearch/vector_db_id_compression rebuilt as hand-written HIP for gfx950 behind a
C-ABI (include/vidc.h); this package is the thin Python host side mirroring the reference's
`custom_invlists` / `altid` SWIG modules.
"""
from . import _lib  # noqa: F401
from ._lib import VIDC_PREC_EXACT, VIDC_PREC_REFERENCE, VidcError  # noqa: F401
from . import persist  # noqa: F401,E402  (save / load of every container: flat .npz images)
from . import removal  # noqa: F401,E402  (removal of (list, id) batches from the list containers)
from . import locate  # noqa: F401,E402  (id -> label: the inverse of translate_labels for the list containers)
from . import merge  # noqa: F401,E402  (two objects over the same lists -> one: Faiss's merge_from)
from . import subset  # noqa: F401,E402  (a part of every list, chosen by rule -> a new object: Faiss's copy_subset_to)
from . import rank  # noqa: F401,E402  (rank, membership and range counts inside compressed Elias-Fano lists and graph rows)

__all__ = ["VidcError", "VIDC_PREC_REFERENCE", "VIDC_PREC_EXACT", "persist", "removal", "locate", "merge", "subset", "rank"]

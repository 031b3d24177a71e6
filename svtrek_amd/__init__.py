"""svtrek_amd -- MI355X-native engine for SVTrek's `audt` SV-refinement hot path.

Product path: include/svtrek_gpu.h (C ABI) implemented by libsvtrek_hip.so (HIP,
gfx950), driven by the `svtrek audt` CLI (csrc/svtrek_main.cpp) or from Python via
Engine.  See DESIGN.md.
"""
from ._lib import (CALL_DTYPE, EVIDENCE_DTYPE, GT_DTYPE, GT_SITE_DTYPE, LOCUS_DTYPE, RESULT_DTYPE, SVT_DEL,  # noqa: F401
                   SVT_INS, SVT_INV, SVT_NA)
from .engine import (Engine, Params, SvtError, calls_to_loci, calls_to_sites, gt_costs, sites_from_loci,  # noqa: F401
                     version)
from .pileup import Pileup, from_reads, make_loci  # noqa: F401

__all__ = ["Engine", "Params", "SvtError", "Pileup", "from_reads", "make_loci", "version", "calls_to_loci", "calls_to_sites",
           "sites_from_loci", "gt_costs", "CALL_DTYPE", "GT_SITE_DTYPE", "GT_DTYPE",
           "LOCUS_DTYPE", "RESULT_DTYPE", "EVIDENCE_DTYPE", "SVT_DEL", "SVT_INS", "SVT_INV", "SVT_NA"]

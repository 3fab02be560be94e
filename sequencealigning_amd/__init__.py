"""sequencealigning_amd — MI355X-native drop-in engine for the NW-affine hot
and WFA paths of Qw11111111111/SequenceAligning (src/needleman_wunsch_affine.rs,
src/wfa.rs).

Compute lives in ``libsaln.so`` (HIP kernels for gfx950 behind the C ABI in
``include/saln.h``); this package is the host-side mirror of the reference's
interface: ``parse_fasta``/``Record``/``Mode`` (src/parse.rs), the
``AlignerError`` family (src/errors.rs), ``n_w_align`` and ``wfa_align``.
"""
from .records import (AlignerError, AlignmentError, Algo, CharError, FastaError, Mode, Record,
                      Records, parse_fasta, parse_fasta_bytes)
from .nw import (NwAlignment, NwAllVsAll, NwPlan, alignment_rows, cigar_ops_string, dense_mask, n_w_align,
                 nw_align_batch, nw_score_all_vs_all, pack_csr, render, render_batch)
from . import wfa
from .wfa import WfaAlignment, WfaPlan, wfa_align, wfa_align_batch
from . import wfa_affine
from .wfa_affine import wfa_affine_align, wfa_affine_align_batch
from . import ends_free
from .ends_free import (EndsFreePlan, EndsFreeScorePlan, SubstitutionMatrix, alignment_score, ends_free_align_batch,
                        ends_free_align_long_batch, extend_align, extend_align_long, local_align, local_align_long, overlap_align,
                        overlap_align_long, semi_global_align, semi_global_align_long, xdrop_extend_long, xdrop_extend_long_batch,
                        xdrop_steps)
from ._lib import get_option, option_names, options, set_option

__all__ = [
    "AlignerError", "AlignmentError", "Algo", "CharError", "FastaError", "Mode", "Record",
    "Records", "parse_fasta", "parse_fasta_bytes", "NwAlignment", "NwPlan", "alignment_rows",
    "cigar_ops_string", "dense_mask", "n_w_align", "NwAllVsAll", "nw_score_all_vs_all", "nw_align_batch", "pack_csr", "render", "render_batch",
    "wfa", "WfaAlignment", "WfaPlan", "wfa_align", "wfa_align_batch", "wfa_affine",
    "wfa_affine_align", "wfa_affine_align_batch",
    "ends_free", "EndsFreePlan", "EndsFreeScorePlan", "SubstitutionMatrix", "alignment_score", "ends_free_align_batch", "local_align", "semi_global_align",
    "ends_free_align_long_batch", "local_align_long", "semi_global_align_long",
    "overlap_align", "overlap_align_long", "extend_align", "extend_align_long", "xdrop_steps",
    "xdrop_extend_long_batch", "xdrop_extend_long",
    "get_option", "option_names", "options", "set_option",
]

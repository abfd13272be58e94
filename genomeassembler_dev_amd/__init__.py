"""genomeassembler_dev_amd — MI355X (gfx950) implementation of the de Bruijn graph construction/traversal and k-meric
breakage-probability scoring hot path of SahakyanLab/GenomeAssembler_dev (lib/DeNovoAssembler.cpp +
lib/BreakageScorer.cpp), behind the reference's own entry points.  Compute is hand-written HIP in libgasm.so, reached
through the C ABI in include/gasm.h; there is no CPU fallback."""
from . import qtable, readkmers, seqio, solutions, synth  # noqa: F401
from ._lib import Context, GasmError, default_context  # noqa: F401
from .api import (ContigMatrix, Scaffolds, align_reads, assemble_contigs, assemble_contigs_velvet, calc_breakscore, calc_breakscore_mapped, calc_breakscore_tables, contig_graph, correct_reads, count_read_kmers,  # noqa: F401
                  coverage_percent, get_contigs, get_contigs_from_fastq, get_contigs_from_reads, get_contigs_from_reads_bubbles, get_contigs_from_reads_simplified, get_kmers_from_reads, levenshtein, map_reads, map_reads_gapped, resolve_repeats, resolve_repeats_paired, unpack_kmers)
from .batch import SegmentBatch  # noqa: F401
from .links import ContigLinks  # noqa: F401
from .pairs import PairPlaces  # noqa: F401
from .readmap import AlignedReadMap, GappedReadMap, MappedScores, ReadMap  # noqa: F401
from .readkmers import r_squared, table_read_kmer_prob  # noqa: F401

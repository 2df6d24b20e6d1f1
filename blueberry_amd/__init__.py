"""blueberry_amd -- MI355X-native replacement for the O(N^2) bin-pair hot path
of jmschrei/blueberry.

Drop-in names (same meaning as in `blueberry.*`, reference
`blueberry/__init__.py:38-43` star-exports):
    count_band_regions            blueberry/blueberry.pyx:77-91
    ContactMap                    blueberry/datatypes.pyx:31-272
    FithicContactMap              blueberry/datatypes.pyx:274-388
    benjamini_hochberg            blueberry/blueberry.pyx:40-75
    downsample                    blueberry/blueberry.pyx:93-104
    Q_LOWER_BOUND, Q_UPPER_BOUND, HIGH_FITHIC_CUTOFF, LOW_FITHIC_CUTOFF
                                  blueberry/utils.py:23-26
Net-new (the reference has no solver; docs/SPEC.md):
    StructureSolver               contact matrix -> 3D coordinates; alpha='auto' infers the
                                  count-to-distance exponent in the fit (SPEC 2.11)
    FitScore                      how well a structure fits a map (SPEC 2.8)
    shortest_paths                sparse map -> complete wish distances (SPEC 2.1.1)
    balance_triples, DeviceTriples
                                  ICE bias and expected straight from a pixel list (SPEC 2.5.3)
    landmark_start, landmark_coefficients, GeodesicRows
                                  a start for sparse maps that holds the global fold: landmark MDS
                                  over device shortest paths from a pixel list (SPEC 2.1.2, 2.5.4)
    FitHiC, binomial_sf           Fit-Hi-C p- and q-values of a resident raw map (SPEC 2.9; the
                                  computation of blueberry/fithic.py:76-108 without its files)
    q_values                      Benjamini-Hochberg q-values of p-values in any order: stable
                                  sort, scan and scatter on the device (SPEC 2.9.7)
    compare_structures, StructureComparison
                                  structure against structure: superposition up to a mirror image,
                                  pair distances per separation and per bin, Spearman ranks by the
                                  device's sort (SPEC 2.10)
    ContactMap.coarsen, DeviceTriples.coarsen, coarsen_triples
                                  a map pooled to a coarser resolution on the device, dense and
                                  pixel list, the same bits (SPEC 2.12)
    coarsen_structure, prolong_structure
                                  a structure between two resolutions, host numpy (SPEC 2.12)
    ContactMap.insulation, DeviceTriples.insulation, insulation_triples, InsulationTrack
                                  the insulation score of a map and its domain (TAD) boundaries:
                                  a banded pass on the device, dense and pixel list, the same
                                  bits; score, log2 and boundary strengths in numpy (SPEC 2.13)

All compute runs in libblueberry_hip.so (hand-written HIP for gfx950) behind
the C-ABI of include/blueberry_hip.h.  Importing this package needs neither
the library nor a GPU; the first compute call does, and raises if either is
missing -- there is no CPU fallback.
"""
from .utils import (HIGH_FITHIC_CUTOFF, LOW_FITHIC_CUTOFF, Q_LOWER_BOUND,  # noqa: F401
                    Q_UPPER_BOUND)
from .band import count_band_regions  # noqa: F401
from .datatypes import (ContactMap, EigenNoConvergence, FithicContactMap,  # noqa: F401
                        InsulationTrack, shortest_paths)
from .compare import StructureComparison, compare_structures  # noqa: F401
from .engine import HipEngine, RankDeficient  # noqa: F401
from .fithic import FitHiC, binomial_sf  # noqa: F401
from .landmark import landmark_coefficients, landmark_start  # noqa: F401
from .resolution import coarsen_structure, prolong_structure  # noqa: F401
from .solver import FitScore, StructureSolver  # noqa: F401
from .stats import benjamini_hochberg, downsample, q_values  # noqa: F401
from .triples import (DeviceTriples, GeodesicRows, TriplesBalance, balance_triples,  # noqa: F401
                      coarsen_triples, insulation_triples)

__version__ = "0.1.0"

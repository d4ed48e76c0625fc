"""Physical constants: the MetPy 1.6.2 values the reference uses (thermodynamics.py:21-22,
conversion_terms.py:31, boundary_terms.py:31, energy_contents.py:31 of the reference).
They must agree with lorenzcycletoolkit_amd/csrc/lec_internal.h."""
G = 9.80665
RE = 6371008.7714
RD = 8.314462618 / 28.96546e-3
CP_D = 1.4 * RD / (1.4 - 1.0)
KAPPA = RD / CP_D
P0_PA = 100000.0

# column order of the `scalars` output of lec_reduce (include/lec_hip.h: LEC_NSCALAR)
SCALAR_TERMS = ["Az", "Ae", "Kz", "Ke", "Cz", "Ca", "Ck", "Ce",
                "BAz", "BAe", "BKz", "BKe", "BΦZ", "BΦE", "Gz", "Ge"]
# table order of the `levels` output (lec_fixed_framework.py:172-194 of the reference)
LEVEL_TERMS = ["Az", "Ae", "Kz", "Ke", "Ge", "Gz", "Cz", "Cz_1", "Cz_2", "Ca", "Ca_1", "Ca_2",
               "Ce", "Ce_1", "Ce_2", "Ck", "Ck_1", "Ck_2", "Ck_3", "Ck_4", "Ck_5"]
# the terms that have a latitude-pressure section (LECResult.section_*; lec_sections), in the kernel's order
SECTION_TERMS = ["Az", "Ae", "Kz", "Ke", "Cz", "Ca", "Ck", "Ce", "Gz", "Ge"]
# the eddy terms that have a longitude-resolved map (LECResult.map_*; lec_maps), in the kernel's order; the zonal terms have no
# longitude structure
MAP_TERMS = ["Ae", "Ke", "Ca", "Ce", "Ck", "Ge"]
# the eddy terms that have a zonal-wavenumber spectrum (LECResult.spectrum) and their per-level tables (LECResult.spectrum_levels;
# Ce_1 = Rd / (p g) is a function of level alone, the same for every wavenumber: carried so that Ce's pieces stay together)
SPECTRUM_TERMS = ["Ae", "Ke", "Ca", "Ce", "Ck"]
SPECTRUM_LEVEL_TERMS = ["Ae", "Ke", "Ca", "Ca_1", "Ca_2", "Ce", "Ce_1", "Ce_2", "Ck", "Ck_1", "Ck_2", "Ck_3", "Ck_4", "Ck_5"]
# the generation term whose spectrum is asked for separately (LECResult.spectrum_ge / spectrum_ge_levels: it costs a kernel of its own,
# lec_rowspec_q_ring, because Q never reaches a row record); a scalar and a per-level table of the same name
SPECTRUM_GENERATION_TERM = "Ge"
# the non-linear eddy-eddy transfers (LECResult.spectrum_nl / spectrum_nl_levels; lec_rowspec_nl_ring): S(n) into Ae and L(n) into Ke, and
# the places of stage 2 they are read from (Ae is linear in [T'T'], Ke in [u'u'] + [v'v'])
SPECTRUM_INTERACTION_TERMS = ["S", "L"]
SPECTRUM_INTERACTION_PLACES = ["Ae", "Ke"]
# the per-wavenumber budget of the eddy reservoirs (LECResult.spectrum_b / spectrum_tendency / spectrum_residual; lec_rowspec_b_ring):
# the boundary terms read from their own places of stage 2, the finite-difference tendencies and the residuals of the reference's budget
SPECTRUM_BUDGET_TERMS = ["BAe", "BKe"]
SPECTRUM_TENDENCY_TERMS = ["Ae", "Ke"]
SPECTRUM_TENDENCY_FILES = ["dAedt", "dKedt"]
SPECTRUM_RESIDUAL_TERMS = ["RGe", "RKe"]

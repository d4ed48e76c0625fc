#!/usr/bin/env python3
"""Lorenz Energy Cycle (LEC) program -- MI355X-native engine behind the command line of
daniloceano/LorenzCycleToolkit (reference lorenzcycletoolkit.py:50-265).

Same flags, same ``inputs/namelist`` / ``inputs/box_limits`` / track files, same
``./LEC_Results/<infile>_<method>/`` tree and CSV schema; the numerics run as HIP kernels on the GPU
(``lorenzcycletoolkit_amd``).  Out of scope: plots (-p), the interactive
map of the domain chooser, CDS-API downloads (--cdsapi).

-c/--choose runs without a display: instead of waiting for clicks on a map, the GPU follows the 850-hPa system from time step to
time step (``lec_follow``; --choose-start, --choose-box, --choose-search, --choose-smooth, --choose-field, --choose-hemisphere,
--choose-domain), writes the boxes' centres as a track file to ``LEC_Results/<infile>_choose/<infile>_choose_track`` and then
runs the moving framework on that track -- the very run ``-t --trackfile <that file>`` does, under the chooser's file names.
With --choose-systems K (or --choose-starts FILE) it finds the K strongest systems of the first time step (``lec_follow_seeds``),
follows them all in one launch (``lec_follow_many``), writes ``LEC_Results/<infile>_choose_batch/choose_s01``, ``choose_s02``, ... and
is from there on ``-t --trackfiles <those files>``: one tree ``LEC_Results/<infile>_choose_sNN_track/`` per system.
With --batch-chunk N a batch of tracks (of either kind) is analysed from the streamed file, N time steps of the tracks' union resident per
pipeline slot (``ingest.lec_streamed_batch``), instead of from a union of all tracks' steps and crops prepared on the host: the same files.
With --choose-lifecycle (and --choose-threshold X) every time step is searched (``lec_follow_seeds_series``), a system is followed from
the time step at which it forms until it has weakened (``lec_follow_spans``; --choose-end-threshold, --choose-patience,
--choose-min-steps), and each track covers its system's own time steps.

-f --periodic: the fixed box is a full ring of longitudes (a zonal band, a hemisphere, the globe): the file's longitudes must close the
circle and the box limits span it; zonal means run over the closed axis, d/dlon is centred across the +-180 meridian and no flux
crosses an east or west wall (``lec_rowstats_ring``).  Same output tree, file names and columns as -f.

-f --periodic --wavenumbers N: also the shares of the zonal wavenumbers 1 .. N in the eddy terms Ae, Ke, Ca, Ce and Ck
(``lec_rowspec_ring``; exact by the discrete Parseval identity on the closed axis), written to results_wavenumbers/<term>_n.csv; every
other output file is unchanged.  With --wavenumbers-generation also Ge (``lec_rowspec_q_ring``: Q at every point of a row, projected
beside T), written to results_wavenumbers/Ge_n.csv.  With --wavenumbers-interactions also the non-linear eddy-eddy (triad) transfers S(n)
into Ae and L(n) into Ke (``lec_rowspec_nl_ring``: the advective tendencies at every point of a row, projected beside T, u and v), written
to results_wavenumbers/S_n.csv and L_n.csv in W m-2, positive where wavenumber n gains.  With --wavenumbers-budget also the boundary terms
BAe(n) and BKe(n) (``lec_rowspec_b_ring``: the triple products of a row as covariances of pointwise products, projected beside T, u and
v), the finite-difference tendencies and the residuals RGe(n) and RKe(n) as the results CSV defines them for the totals, written to
results_wavenumbers/BAe_n.csv, BKe_n.csv, dAedt_n.csv, dKedt_n.csv, RGe_n.csv and RKe_n.csv.  With --wavenumbers-chunk M the file is streamed to the GPU, M time steps resident
per pipeline slot, and the spectra are computed chunk by chunk (``lec_level_spec_ring``): the same files, for series that do not fit
the GPU whole.

-f [--periodic] --sections: also the latitude-pressure sections of Az, Ae, Kz, Ke, Cz, Ca, Ck, Ce, Gz, Ge on the box's rows
(``lec_sections``: the row's own contribution to the per-level sums of stage 2), written to results_sections/<term>_lat_lv.csv (the time
mean, levels x latitudes) and <term>_lat.csv (the vertical integral, time steps x latitudes); with --wavenumbers N also <term>_n_lat.csv.

-f [--periodic] --maps: also the longitude-resolved maps of the eddy terms Ae, Ke, Ca, Ce, Ck, Ge on the box's points (``lec_maps``: the
term's integrand with the zonal average left off, integrated over pressure), written to results_maps/<term>_lat_lon.csv (the time mean,
latitudes x longitudes) and <term>_lon.csv (the area-weighted sum over latitude, time steps x longitudes: a Hovmoeller diagram).

-t / -c --composites: also the system-relative composites of the same six eddy terms over the boxes that follow the system
(``lec_composite``: ``lec_maps`` on box-relative points, every step with its own box), written to results_composites/<term>_dlat_dlon.csv
(the time mean, box rows x box columns, labelled by the offset in degrees from the box's midpoint) and <term>_dlon.csv (the area-weighted
sum over the box's rows, time steps x box columns).  One system whose boxes all have one shape.

-t --trackfiles / -c --choose-systems --batch-composites: the composites of EVERY track of a batch in the batch's one pass
(``lec_composite_steps``: ``lec_composite`` on the union cube, every box with its step from the batch's step table, the time sums kept per
track) and their ensemble mean (``lec_composite_ensemble``).  Every track's tree gets the results_composites/ of its own
``-t --trackfile --composites`` run, byte for byte; the batch directory gets results_composites/<term>_dlat_dlon.csv, the mean over the
tracks of their time-mean composites, and composites.csv -- one results_composites_<rows>x<columns>/ per box shape where shapes differ.
--batch-composites-phase lifetime:B | peak:L: also phase-aligned ensembles (``lec_composite_phase_sum``, ``lec_composite_phase_ensemble``):
every track's life cut into B bins, or the tracks aligned on their step of peak |min_max_zeta_850| with L lags on either side; a track
enters a bin's ensemble where it has a step in it.  The ensemble directory gets phases/ (per bin <term>_dlat_dlon_phase<bb>.csv and
<term>_sd_dlat_dlon_phase<bb>.csv, phases.csv, phase_members.csv, phase_terms.csv); nothing else changes.

-f [--periodic] --lon-sections: also the longitude-pressure sections of Ae, Ke, Ca, Ce, Ck, Ge (``lec_lonsections``: the maps' integrand
summed over the box's rows with their area weights instead of over pressure), written to results_lon_sections/<term>_lon_lv.csv (the time
mean, levels x longitudes).  -t / -c --composite-lon-sections: the same on the box-relative columns of the boxes that follow a system
(``lec_composite_lonsections``), written to results_composite_lon_sections/<term>_dlon_lv.csv.  Not for batches, streamed or sharded runs.

-t / -c --composite-sections: also the system-relative latitude-pressure sections of Az, Ae, Kz, Ke, Cz, Ca, Ck, Ce, Gz, Ge over the boxes
that follow the system (``lec_composite_sections``: ``lec_sections`` on box-relative rows, every step with its own box), written to
results_composite_sections/<term>_dlat_lv.csv (the time mean, levels x box rows, labelled by the offset in degrees from the box's
midpoint) and <term>_dlat.csv (the vertical integral, time steps x box rows).  One system whose boxes all have one row count; only the
row records are read, so it runs on the streamed path (--ingest device / --device-ingest) too, and may be combined with --composites.

--series FILE...: the time series that ``infile`` begins continues in these files (archives deliver a file per month or per day): same
grid, levels and variables, time stamps that do not overlap; every file is decoded with its own scale_factor / add_offset (on the GPU:
``lec_ingest_series``, a table of packing constants per time step).  Every output is named after ``infile``.

Several GPUs of one node: ``python lorenzcycletoolkit.py <file> -r -f --gpus N`` (this process starts N rank processes, one per
GPU) or ``python -m torch.distributed.run --nproc-per-node N lorenzcycletoolkit.py <file> -r -f``.  The time steps are sharded
over the ranks (each reads, decodes and computes only its own block plus a one-step halo of T), rank 0 gathers the per-step
results over RCCL and writes the very same files as the one-GPU run.
"""
import argparse
import logging
import os
import sys
import time

import pandas as pd

from lorenzcycletoolkit_amd import phases
from lorenzcycletoolkit_amd.dataset import prepare_data
from lorenzcycletoolkit_amd.frameworks import lec_fixed, lec_moving, lec_moving_batch, lec_moving_batch_streamed

phases.mark("imports")          # interpreter start -> here: Python, pandas, torch and the package


def create_arg_parser():
    """The reference's command line (lorenzcycletoolkit.py:50-129 there): the same flags, defaults and mutual exclusions -- the
    flag table is the drop-in contract; the help texts are this program's own."""
    parser = argparse.ArgumentParser(description="Lorenz Energy Cycle of a limited area, computed on an AMD GPU (MI355X HIP engine).")
    parser.add_argument("infile", help="NetCDF file (classic or NetCDF-4) holding T, u, v, omega and geopotential (or geopotential height) "
                        "on isobaric levels; variable names come from inputs/namelist")
    parser.add_argument("-r", "--residuals", action="store_true", help="close the budgets with residual terms (RGz, RKz, RGe, RKe) instead of "
                        "friction-based dissipation; the only mode the reference completes")
    group = parser.add_mutually_exclusive_group(required=True)
    group.add_argument("-f", "--fixed", action="store_true", help="Eulerian framework: one box for the whole series, read from the box-limits file")
    group.add_argument("-t", "--track", action="store_true", help="semi-Lagrangian framework: one box per time step, centred on the track file's positions")
    group.add_argument("-c", "--choose", action="store_true", help="semi-Lagrangian framework without a track file: the GPU picks each time step's box by "
                       "following the 850-hPa vorticity (or height) extremum from step to step (the reference's interactive map needs a display; "
                       "see the --choose-* options), writes the track it found and analyses it as -t would")
    parser.add_argument("-z", "--zeta", action="store_true", help="with -t: report the 850-hPa vorticity at the track position rather than the box extremum")
    parser.add_argument("-m", "--mpas", action="store_true", help="input comes from MPAS-A post-processed with MPAS-BR")
    parser.add_argument("-p", "--plots", action="store_true", help="accepted for compatibility; figures are made by the reference's plot scripts from the CSVs")
    parser.add_argument("-v", "--verbosity", action="store_true", help="log at DEBUG level")
    parser.add_argument("--cdsapi", action="store_true", help="download ERA5 through the CDS API first (needs network access: not available in this build)")
    parser.add_argument("--time-resolution", type=int, default=3, help="hours between downloaded analyses with --cdsapi (default: 3)")
    parser.add_argument("--trackfile", type=str, default="inputs/track", help="track file for -t (default: inputs/track)")
    parser.add_argument("--trackfiles", nargs="+", metavar="PATH", help="with -t: many track files over the same data file in ONE pass "
                        "(a directory stands for every regular file in it, sorted by name).  Each track writes LEC_Results/<infile>_<track>_track/ "
                        "with the files a --trackfile run of it writes; the log and batch.csv go to LEC_Results/<infile>_track_batch/")
    parser.add_argument("--batch-chunk", type=int, metavar="N", help="with -t --trackfiles (or -c --choose-systems / --choose-starts): stream the "
                        "file to the GPU N time steps of the tracks' union at a time and decode / crop every track's boxes there, instead of "
                        "decoding the union of all tracks' time steps and crops on the host and uploading it whole: device memory then depends "
                        "on N, not on the length of the series (a batch that is refused for its size runs this way), and a deflated NetCDF-4 file "
                        "is inflated on the GPU.  Same output files, byte for byte.  Independent of --choose-chunk")
    parser.add_argument("--box_limits", type=str, default="inputs/box_limits", help="box-limits file for -f (default: inputs/box_limits)")
    parser.add_argument("--periodic", action="store_true", help="with -f: the box is a full ring of longitudes -- a zonal band, a hemisphere, the "
                        "globe.  The file's longitudes must be evenly spaced with nx * dx = 360 degrees and the box limits' min_lon / max_lon must "
                        "select its first and last longitude (-180 / 180 always do); min_lat / max_lat give the band.  Zonal means run over the "
                        "closed circle, d/dlon is centred across the +-180 meridian and no flux crosses an east or west wall (otherwise the "
                        "circle is a limited area with a seam)")
    # (no attribute without the option, as for --series)
    parser.add_argument("--wavenumbers", type=int, metavar="N", default=argparse.SUPPRESS, help="with -f --periodic: also split the eddy terms "
                        "Ae, Ke, Ca, Ce and Ck into the shares of the zonal wavenumbers 1 .. N (N <= nx / 2 and N <= 64) and write them to "
                        "results_wavenumbers/Ae_n.csv ... Ck_n.csv: one row per time step, columns 1 .. N and 'rest' (the total minus the N "
                        "shares), in the units of the results CSV.  The split is exact (discrete Parseval on the closed axis); every other "
                        "output file is unchanged.  One GPU, data prepared on the host (--ingest auto resolves to host)")
    parser.add_argument("--wavenumbers-generation", action="store_true", default=argparse.SUPPRESS, help="with --wavenumbers N: also split the "
                        "generation term Ge and write results_wavenumbers/Ge_n.csv, in the form of its five siblings.  The diabatic-heating "
                        "residual Q is evaluated at every point of the ring's rows once more and projected beside T (lec_rowspec_q_ring)")
    parser.add_argument("--wavenumbers-interactions", action="store_true", default=argparse.SUPPRESS, help="with --wavenumbers N: also the "
                        "non-linear eddy-eddy (triad) transfers S(n) into Ae and L(n) into Ke, written to results_wavenumbers/S_n.csv and L_n.csv "
                        "in the form of their siblings (W m-2, positive: wavenumber n gains; 'rest' is the total, summed in physical space, minus "
                        "the N shares).  The eddy-eddy advective tendencies of T, u and v are evaluated at every point of the ring's rows and "
                        "projected beside T, u and v (lec_rowspec_nl_ring)")
    parser.add_argument("--wavenumbers-budget", action="store_true", default=argparse.SUPPRESS, help="with --wavenumbers N: also the budget of "
                        "every wavenumber's Ae and Ke on the open band: the boundary terms BAe(n) and BKe(n) (the flux through the band's north "
                        "and south walls and through its top and bottom level), the tendencies dAe(n)/dt and dKe(n)/dt (np.gradient with the "
                        "run's dt: the series needs at least 2 time steps) and the residuals RGe(n) = dAe/dt - Ca + Ce - BAe and RKe(n) = dKe/dt "
                        "- Ce + Ck - BKe, written to results_wavenumbers/BAe_n.csv, BKe_n.csv, dAedt_n.csv, dKedt_n.csv, RGe_n.csv and RKe_n.csv "
                        "in the form of their siblings.  The four triple products behind BAe and BKe are split as covariances of pointwise "
                        "products (lec_rowspec_b_ring)")
    parser.add_argument("--wavenumbers-chunk", type=int, metavar="N", default=argparse.SUPPRESS, help="with --wavenumbers: stream the file to the "
                        "GPU with N time steps resident per pipeline slot and compute the spectra chunk by chunk (lec_level_spec_ring), instead "
                        "of preparing the whole series on the host and holding it on the GPU: device memory then depends on N, not on the "
                        "length of the series, and a deflated NetCDF-4 file is inflated on the GPU.  Same output files, byte for byte")
    parser.add_argument("--sections", action="store_true", default=argparse.SUPPRESS, help="with -f [--periodic]: also the latitude-pressure "
                        "sections of the ten terms Az, Ae, Kz, Ke, Cz, Ca, Ck, Ce, Gz and Ge (lec_sections), written to results_sections/: "
                        "<term>_lat_lv.csv, the time mean of the term's section (rows: levels, columns: the box's latitudes; its "
                        "area-weighted sum over the latitudes is the term's per-level table) and <term>_lat.csv, the vertical integral at "
                        "every time step (rows: time steps, in the units of the results CSV).  With --wavenumbers N also <term>_n_lat.csv "
                        "for the spectral terms: the time mean of the vertical integral of every wavenumber's share (rows 1 .. N and "
                        "'rest').  Every other output file is unchanged.  One GPU; not for -t / -c")
    parser.add_argument("--maps", action="store_true", default=argparse.SUPPRESS, help="with -f [--periodic]: also the longitude-resolved maps "
                        "of the six eddy terms Ae, Ke, Ca, Ce, Ck and Ge (lec_maps: the term's integrand at every point of the box, the zonal "
                        "average left off, integrated over pressure), written to results_maps/: <term>_lat_lon.csv, the time mean (rows: the "
                        "box's latitudes, columns: its longitudes, in the units of the results CSV; the box's zonal average of a row is the "
                        "term's --sections column) and <term>_lon.csv, the area-weighted sum over latitude at every time step (rows: time "
                        "steps, columns: longitudes: a Hovmoeller diagram whose zonal average is the results CSV).  The zonal terms have no "
                        "longitude structure and no map.  Every other output file is unchanged.  One GPU, data prepared on the host "
                        "(--ingest auto resolves to host), evenly spaced longitudes; not for -t / -c")
    parser.add_argument("--composites", action="store_true", default=argparse.SUPPRESS, help="with -t --trackfile or -c (one system): also "
                        "the system-relative composites of the six eddy terms Ae, Ke, Ca, Ce, Ck and Ge (lec_composite: the term's integrand at "
                        "every point of every time step's box, integrated over pressure, laid on the box-relative points), written to "
                        "results_composites/: <term>_dlat_dlon.csv, the time mean over the system's life (rows: the box's rows, columns: its "
                        "columns, both labelled by the offset in degrees from the box's midpoint, in the units of the results CSV) and "
                        "<term>_dlon.csv, the area-weighted sum over the box's rows at every time step (rows: time steps; the box's zonal "
                        "average of a row is the results CSV).  Every other output file is unchanged.  One GPU, data prepared on the host "
                        "(--ingest auto resolves to host), evenly spaced longitudes and latitudes, boxes of one shape; -f has --maps")
    parser.add_argument("--lon-sections", dest="lon_sections", action="store_true", default=argparse.SUPPRESS,
                        help="with -f [--periodic]: also the longitude-pressure sections of the six eddy terms Ae, Ke, Ca, Ce, Ck and Ge "
                        "(lec_lonsections: the term's integrand at every point of the box, summed over the box's rows with their area "
                        "weights), written to results_lon_sections/<term>_lon_lv.csv: the time mean (rows: the levels, columns: the box's "
                        "longitudes in degrees) in the units of --sections' <term>_lat_lv.csv.  Its zonal average is the row-weighted sum "
                        "of --sections, its vertical integral the Hovmoeller of --maps.  One GPU, data prepared on the host (--ingest auto "
                        "resolves to host), evenly spaced longitudes, at least 3 of them; may be combined with --maps, --sections, "
                        "--wavenumbers, --series and -r; -t / -c have --composite-lon-sections")
    parser.add_argument("--composite-lon-sections", dest="composite_lon_sections", action="store_true", default=argparse.SUPPRESS,
                        help="with -t --trackfile or -c (one system): also the system-relative longitude-pressure sections of the same six "
                        "eddy terms over the boxes that follow the system (lec_composite_lonsections), written to "
                        "results_composite_lon_sections/<term>_dlon_lv.csv: the time mean over the system's life (rows: the levels, "
                        "columns: the box's columns, labelled by the offset in degrees from the box's midpoint).  What --composites needs: "
                        "one GPU, data prepared on the host, evenly spaced longitudes and latitudes, boxes of one shape; may be combined "
                        "with --composites and --composite-sections; -f has --lon-sections")
    parser.add_argument("--batch-composites", dest="batch_composites", action="store_true", default=argparse.SUPPRESS,
                        help="with -t --trackfiles or -c --choose-systems / --choose-starts (a batch of tracks): the composites of EVERY track "
                        "in the batch's one pass (lec_composite_steps) and their ensemble mean (lec_composite_ensemble).  Every track's tree "
                        "gets results_composites/, byte for byte what -t --trackfile <it> --composites writes; the batch directory gets "
                        "results_composites/<term>_dlat_dlon.csv, the mean over the tracks of their time-mean composites, and composites.csv "
                        "(per track: its file, steps, box shape and the NaN points of its mean) -- one results_composites_<rows>x<columns>/ per "
                        "box shape where the tracks' shapes differ.  Every other output file is unchanged.  Every track needs boxes of one "
                        "shape along its life and evenly spaced longitudes and latitudes on its own crop.  One GPU, data prepared on the "
                        "host (--ingest auto resolves to host); not with --batch-chunk; one system has --composites")
    parser.add_argument("--batch-composites-phase", dest="batch_composites_phase", metavar="lifetime:B|peak:L", default=argparse.SUPPRESS,
                        help="with --batch-composites: also PHASE-ALIGNED ensembles of the composites (lec_composite_phase_sum, "
                        "lec_composite_phase_ensemble).  A clock gives every track B ranges of its own steps.  lifetime:B cuts every track's "
                        "life into B bins, step s of n in bin (s * B) // n; peak:L aligns the tracks on their step of peak intensity -- the "
                        "first step at which |min_max_zeta_850| of the track's *_trackfile is largest -- and takes the 2 L + 1 lags -L .. +L in "
                        "steps (the tracks need one common, even time spacing).  A track enters a bin's ensemble where it has a step in it.  "
                        "The ensemble directory gets phases/: <term>_dlat_dlon_phase<bb>.csv (the mean over the bin's tracks of their means "
                        "over the bin) and <term>_sd_dlat_dlon_phase<bb>.csv (their n - 1 standard deviation) per bin, phases.csv, "
                        "phase_members.csv and phase_terms.csv (the results CSVs' columns averaged the same way).  No other file changes")
    parser.add_argument("--composite-sections", dest="composite_sections", action="store_true", default=argparse.SUPPRESS,
                        help="with -t --trackfile or -c (one system): also the system-relative latitude-pressure sections of the ten terms "
                        "Az, Ae, Kz, Ke, Cz, Ca, Ck, Ce, Gz and Ge (lec_composite_sections: the row's own contribution to the per-level sums "
                        "of every time step's box, laid on the box-relative rows), written to results_composite_sections/: "
                        "<term>_dlat_lv.csv, the time mean over the system's life (rows: levels, columns: the box's rows labelled by the "
                        "offset in degrees from the box's midpoint, in the units of the per-level tables) and <term>_dlat.csv, the vertical "
                        "integral at every time step (rows: time steps, in the units of the results CSV).  Every other output file is "
                        "unchanged.  One GPU, host-prepared or streamed data, evenly spaced latitudes, boxes of one row count (their widths "
                        "may differ); may be combined with --composites; -f has --sections")
    parser.add_argument("--device-ingest", action="store_true", help="stream the file's bytes to the GPU in chunks and decode / sort / crop them "
                        "there, instead of preparing the whole data set on the host (same results, bit for bit); the same as --ingest device")
    parser.add_argument("--ingest", choices=["auto", "host", "device"], default="auto", help="where the data are prepared: 'host' decodes, sorts "
                        "and crops with NumPy and uploads the cubes; 'device' streams the file's bytes and does it on the GPU; 'auto' (default) "
                        "takes the device for deflated NetCDF-4 files whose chunks the GPU can inflate (the host inflates them ten times "
                        "slower) and for any file of 1 GiB or more that the streamed path can read, the host otherwise -- the output files "
                        "are the same, byte for byte")
    parser.add_argument("--inflate", choices=["auto", "host", "device"], default="auto", help="with --device-ingest and a chunked NetCDF-4 file: where "
                        "the (deflated) chunks are inflated -- on the GPU (lec_inflate; the default wherever the variables allow it) or on the host's threads")
    parser.add_argument("--vorticity-form", choices=["metpy_no_crs", "spherical"], default="metpy_no_crs", help="with -t: formulation of the 850-hPa "
                        "relative vorticity in the trackfile (default: what MetPy 1.6.2 evaluates for data without a CRS, as the reference passes them)")
    parser.add_argument("--choose-domain", metavar="FILE", help="with -c: box-limits file of the domain the system is searched in (default: the file's whole domain)")
    parser.add_argument("--choose-start", nargs=2, type=float, metavar=("LAT", "LON"), help="with -c: where the system is at the first time step "
                        "(default: the extremum of the whole search domain)")
    parser.add_argument("--choose-box", nargs=2, type=float, metavar=("LENGTH", "WIDTH"), help="with -c: the box's size in degrees of latitude / longitude (default: 15 15)")
    parser.add_argument("--choose-search", type=float, metavar="DEG", help="with -c: the largest move of the box's centre per time step, in degrees (default: 5)")
    parser.add_argument("--choose-smooth", type=int, metavar="N", help="with -c: follow the mean over (2N + 1) x (2N + 1) grid points instead of the point values (default: 0)")
    parser.add_argument("--choose-field", choices=["zeta", "hgt"], help="with -c: follow the 850-hPa relative vorticity (default; formulation of "
                        "--vorticity-form) or the geopotential height minimum")
    parser.add_argument("--choose-hemisphere", choices=["south", "north"], help="with -c and the vorticity: follow the minimum (south) or the maximum "
                        "(north); default: south when the search domain's southern edge lies south of the equator")
    parser.add_argument("--choose-chunk", type=int, metavar="N", help="with -c: hold the 850-hPa slices of N time steps at a time, in host memory and "
                        "on the GPU (lec_follow_spans_chunk resumes every system from chunk to chunk); the tracks are those of the run without it.  "
                        "Default: the whole series when its slices fit 2 GiB, otherwise the largest equal chunks that do")
    parser.add_argument("--choose-periodic", action="store_true", default=None, help="with -c: the search domain is a full ring of longitudes "
                        "(evenly spaced, nx * dx = 360 degrees; --choose-domain may still cut latitudes): the system is found and followed "
                        "across the +-180 meridian, where the sorted axis has its seam (otherwise refused, with the domain's extent)")
    parser.add_argument("--choose-systems", type=int, metavar="K", help="with -c: find the (at most) K strongest systems of the first time step, follow "
                        "them all at once and analyse every one as -t --trackfiles would: the tracks choose_s01, choose_s02, ..., systems.csv, the log "
                        "and batch.csv go to LEC_Results/<infile>_choose_batch/, each system's results to LEC_Results/<infile>_choose_sNN_track/")
    parser.add_argument("--choose-threshold", type=float, metavar="X", help="with --choose-systems: only systems at least as strong as X, in the field's "
                        "own unit AND sign (1/s for zeta, gpm for hgt): the southern-hemisphere vorticity minimum wants a negative number, e.g. -5e-5")
    parser.add_argument("--choose-separation", nargs=2, type=float, metavar=("LAT_DEG", "LON_DEG"), help="with --choose-systems: a system is the "
                        "best value within this many degrees of latitude / longitude around it (default: half the box)")
    parser.add_argument("--choose-starts", metavar="FILE", help="with -c: follow the systems that are, at the first time step, at the positions "
                        "of this Lat;Lon file (one row per system) instead of finding them; otherwise as --choose-systems")
    parser.add_argument("--choose-lifecycle", action="store_true", default=None, help="with --choose-systems K and --choose-threshold X: systems may "
                        "form after the first time step and end before the last.  Every time step is searched for (at most K) systems; one that no "
                        "system of the step before explains is followed from its own time step on, until it has been weaker than "
                        "--choose-end-threshold for --choose-patience time steps in a row.  Each track covers its system's own time steps; "
                        "systems.csv has a row per system found")
    parser.add_argument("--choose-end-threshold", type=float, metavar="X", help="with --choose-lifecycle: a followed system is alive while it is at "
                        "least as strong as X (unit and sign as --choose-threshold, which is the default; X may be weaker than it, never stricter)")
    parser.add_argument("--choose-patience", type=int, metavar="N", help="with --choose-lifecycle: a system ends after N time steps in a row below "
                        "--choose-end-threshold (default: 2); its track ends at the last time step at which it was strong enough")
    parser.add_argument("--choose-min-steps", type=int, metavar="N", help="with --choose-lifecycle: systems that live for fewer than N time steps "
                        "are listed in systems.csv but not analysed (default and least value: 2)")
    parser.add_argument("--gpus", type=int, default=1, help="shard the time steps over this many GPUs of the node (one process per GPU, "
                        "results gathered over RCCL; same output files).  Under torch.distributed.run the launcher's WORLD_SIZE counts")
    parser.add_argument("-o", "--outname", type=str, help="name of the results CSV (fixed framework)")
    # (no attribute without the option: the logged Namespace of a run without --series is what it was)
    parser.add_argument("--series", nargs="+", metavar="FILE", default=argparse.SUPPRESS, help="the time series that infile begins continues in "
                        "these files (one per month or day, as archives deliver them): same grid, levels and variables, time stamps that do not "
                        "overlap; each file may pack its values with its own scale_factor / add_offset.  Any order (the files are ordered by "
                        "their first time stamp); infile may be named again, so 'a_01.nc --series a_*.nc' works.  Every output is named after "
                        "infile, as for one merged file of that name.  With -f, -t, --trackfiles and -c, --ingest host / device and --gpus N")
    return parser


def refuse_series_options(args):
    """What a --series run does not do, said before anything is created."""
    if getattr(args, "series", None) is None:
        return
    if args.cdsapi:
        raise SystemExit("--series names files that exist; --cdsapi downloads one: give one of the two")
    if args.inflate == "device":
        raise SystemExit("--series: the device inflate reads one file's chunk index, so the deflated parts of a series are inflated by the "
                         "reader on the host: --inflate device is not supported with --series (leave it out, or --inflate host)")


def setup_results_directory(args, method):
    """Reference lorenzcycletoolkit.py:132-155."""
    results_subdirectory = os.path.join("./LEC_Results/", "".join(args.infile.split("/")[-1].split(".nc")) + "_" + method)
    results_subdirectory_vertical_levels = os.path.join(results_subdirectory, "results_vertical_levels")
    figures_directory = os.path.join(results_subdirectory, "Figures")
    os.makedirs(figures_directory, exist_ok=True)
    os.makedirs(results_subdirectory, exist_ok=True)
    os.makedirs(results_subdirectory_vertical_levels, exist_ok=True)
    return results_subdirectory, figures_directory, results_subdirectory_vertical_levels


def _leave_only_the_log(results_subdirectory):
    """A run that failed leaves no half-written results behind.  Like the reference, the results tree is created BEFORE the input is
    read (lorenzcycletoolkit.py:250-258 there), so a file the reader refuses, a bad namelist or a failure in mid-analysis would
    leave empty directories and header-only CSVs that look like results.  When THIS run created the tree, everything but the log --
    which carries the error -- is removed again; a tree that existed before (earlier results) is not touched."""
    import shutil
    for name in os.listdir(results_subdirectory):
        path = os.path.join(results_subdirectory, name)
        if name.startswith("log."):
            continue
        if os.path.isdir(path):
            shutil.rmtree(path, ignore_errors=True)
        else:
            try:
                os.remove(path)
            except OSError:
                pass


def initialize_logging(results_subdirectory, args):
    """Reference src/utils/tools.py:32-73: logger "lorenzcycletoolkit", file log.<stem> + console.  In a time-sharded run only
    rank 0 logs to the file; the other ranks report warnings and errors on the console."""
    level = logging.DEBUG if args.verbosity else logging.INFO
    logger = logging.getLogger("lorenzcycletoolkit")
    logger.setLevel(level)
    for h in list(logger.handlers):
        logger.removeHandler(h)
    fmt = logging.Formatter("%(asctime)s - %(name)s - %(levelname)s - %(message)s")
    shard = getattr(args, "shard", None)
    if shard is not None and not shard.root:
        ch = logging.StreamHandler()
        ch.setFormatter(logging.Formatter(f"%(asctime)s - rank {shard.rank} - %(levelname)s - %(message)s"))
        ch.setLevel(logging.WARNING)
        logger.addHandler(ch)
        return logger
    stem = os.path.basename(args.infile).split(".nc")[0]
    fh = logging.FileHandler(os.path.join(results_subdirectory, f"log.{stem}"), mode="w")
    fh.setFormatter(fmt)
    ch = logging.StreamHandler()
    ch.setFormatter(fmt)
    logger.addHandler(fh)
    logger.addHandler(ch)
    return logger


def run_lec_analysis(data, args, results_subdirectory, figures_directory, results_subdirectory_vertical_levels, app_logger):
    """Reference lorenzcycletoolkit.py:158-200."""
    start_time = time.time()
    variable_list_df = pd.read_csv("inputs/namelist", sep=";", index_col=0, header=0)
    if args.fixed:
        lec_fixed(data, variable_list_df, results_subdirectory, results_subdirectory_vertical_levels, app_logger, args)
        app_logger.info("Analysis complete! Fixed framework ran in %.2f seconds" % (time.time() - start_time))
    if args.track or args.choose:
        # dT/dt over the (track-selected) time axis is formed on the device inside the engine
        lec_moving(data, variable_list_df, None, results_subdirectory, figures_directory,
                   results_subdirectory_vertical_levels, app_logger, args)
        app_logger.info("Analysis complete! Moving framework ran in %.2f seconds" % (time.time() - start_time))


CHOOSE_OPTIONS = ("choose_domain", "choose_start", "choose_box", "choose_search", "choose_smooth", "choose_field", "choose_hemisphere",
                  "choose_systems", "choose_threshold", "choose_separation", "choose_starts", "choose_lifecycle", "choose_end_threshold",
                  "choose_patience", "choose_min_steps", "choose_chunk", "choose_periodic")


def refuse_choose_options(args):
    """What goes with -c only, and what a -c run does not do, said before anything is created."""
    given = ["--" + o.replace("_", "-") for o in CHOOSE_OPTIONS if getattr(args, o) is not None]
    if given and not args.choose:
        raise SystemExit(f"{', '.join(given)} go{'es' if len(given) == 1 else ''} with -c/--choose")
    if not args.choose:
        return
    many = args.choose_systems is not None or args.choose_starts is not None
    if args.choose_systems is not None and args.choose_starts is not None:
        raise SystemExit("--choose-systems finds the systems, --choose-starts names them: give one of the two")
    if many and args.choose_start is not None:
        raise SystemExit("--choose-start is the one system of a plain -c run: with --choose-systems / --choose-starts leave it out "
                         "(--choose-starts FILE takes any number of starts)")
    for o in ("choose_threshold", "choose_separation"):
        if getattr(args, o) is not None and args.choose_systems is None:
            raise SystemExit(f"--{o.replace('_', '-')} goes with --choose-systems")
    for o in ("choose_end_threshold", "choose_patience", "choose_min_steps"):
        if getattr(args, o) is not None and not args.choose_lifecycle:
            raise SystemExit(f"--{o.replace('_', '-')} goes with --choose-lifecycle")
    if args.choose_lifecycle:
        if args.choose_starts is not None:
            raise SystemExit("--choose-lifecycle finds the systems of every time step itself: --choose-starts names those of the first, leave it out")
        if args.choose_systems is None or args.choose_threshold is None:
            raise SystemExit("--choose-lifecycle needs --choose-systems K and --choose-threshold X: without a threshold every local extremum "
                             "of every time step is a system")
        if args.choose_patience is not None and args.choose_patience < 1:
            raise SystemExit("--choose-patience must be >= 1 time steps")
        if args.choose_min_steps is not None and args.choose_min_steps < 2:
            raise SystemExit("--choose-min-steps must be >= 2: a track has at least two time steps")
        # stricter than --choose-threshold?  Where the options alone say which way "stronger" points, said here; otherwise the data's
        # hemisphere decides and follow.write_lifecycle_tracks refuses
        smaller_is_stronger = True if args.choose_field == "hgt" else {None: None, "south": True, "north": False}[args.choose_hemisphere]
        if args.choose_end_threshold is not None and smaller_is_stronger is not None and (
                args.choose_end_threshold < args.choose_threshold if smaller_is_stronger else args.choose_end_threshold > args.choose_threshold):
            raise SystemExit(f"--choose-end-threshold {args.choose_end_threshold} is stricter than --choose-threshold {args.choose_threshold}: "
                             "it may be weaker, never stricter")
    if many and (args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        stem = "".join(args.infile.split("/")[-1].split(".nc"))
        raise SystemExit("-c/--choose follows the systems on one GPU (chains over the time steps): run -c once, then "
                         f"-t --trackfile LEC_Results/{stem}_choose_batch/choose_sNN --gpus N for the sharded analysis of a track it wrote")
    if many and (args.ingest == "device" or args.device_ingest) and args.batch_chunk is None:
        raise SystemExit("-c --choose-systems / --choose-starts prepares the data on the host: --ingest device / --device-ingest is not supported "
                         "for a batch of tracks (--batch-chunk N streams the batch to the GPU)")
    if args.choose_systems is not None and not 1 <= args.choose_systems <= 256:
        raise SystemExit("--choose-systems must be 1..256")
    if args.choose_separation is not None and min(args.choose_separation) <= 0:
        raise SystemExit("--choose-separation LAT_DEG LON_DEG must be positive")
    if args.choose_starts is not None and not os.path.exists(args.choose_starts):
        raise SystemExit(f"--choose-starts: {args.choose_starts} not found")
    if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        stem = "".join(args.infile.split("/")[-1].split(".nc"))
        raise SystemExit("-c/--choose follows the system on one GPU (a chain over the time steps): run -c once, then "
                         f"-t --trackfile LEC_Results/{stem}_choose/{stem}_choose_track --gpus N for the sharded analysis of the track it wrote")
    if args.choose_chunk is not None and args.choose_chunk < 1:
        raise SystemExit("--choose-chunk must be >= 1 time steps")
    if args.choose_box is not None and min(args.choose_box) <= 0:
        raise SystemExit("--choose-box LENGTH WIDTH must be positive")
    if args.choose_search is not None and not args.choose_search > 0:
        raise SystemExit("--choose-search must be > 0 degrees")
    if args.choose_smooth is not None and args.choose_smooth < 0:
        raise SystemExit("--choose-smooth must be >= 0 grid points")
    if args.choose_domain is not None and not os.path.exists(args.choose_domain):
        raise SystemExit(f"--choose-domain: {args.choose_domain} not found")


def refuse_periodic_options(args):
    """--periodic is the fixed framework's ring; said before anything is created."""
    if args.periodic and not args.fixed:
        raise SystemExit("--periodic goes with -f/--fixed: the ring of a -t / -c run is the 0..360 longitude axis a track across the +-180 "
                         "meridian gets by itself, and --choose-periodic for the search of -c")
    if getattr(args, "sections", False):
        if not args.fixed:
            raise SystemExit("--sections goes with -f/--fixed: a section lies on the rows of ONE fixed box; the boxes of a -t / -c run "
                             "move, and their sections would be system-relative composites")
        if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("--sections runs on one GPU: --gpus > 1 is not supported for the sections (run the totals sharded, the sections apart)")
    if getattr(args, "maps", False):
        if not args.fixed:
            raise SystemExit("--maps goes with -f/--fixed: a map lies on the points of ONE fixed box; the boxes of a -t / -c run move, "
                             "and their maps would be system-relative composites")
        if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("--maps runs on one GPU: --gpus > 1 is not supported for the maps (run the totals sharded, the maps apart)")
        if getattr(args, "wavenumbers_chunk", None) is not None:
            raise SystemExit("--maps prepares the data on the host: --wavenumbers-chunk streams the series and is not supported for the maps "
                             "(the maps read the field cubes once more)")
        if args.ingest == "device" or args.device_ingest:
            raise SystemExit("--maps prepares the data on the host: --ingest device / --device-ingest is not supported for the maps "
                             "(--ingest auto resolves to host)")
    if getattr(args, "composites", False):
        if args.fixed:
            raise SystemExit("--composites goes with -t / -c: ONE fixed box has --maps, the maps on the box's own points; a composite is "
                             "laid on the box-relative points of the boxes that follow a system")
        if args.trackfiles is not None:
            raise SystemExit("--composites follows ONE system: --trackfiles analyses a batch of tracks and has no composites "
                             "(run -t --trackfile FILE --composites for the track that matters)")
        if args.choose and (args.choose_systems is not None or args.choose_starts is not None):
            raise SystemExit("--composites follows ONE system: -c --choose-systems / --choose-starts follows a batch and has no composites "
                             "(run -t --trackfile on a track it wrote, with --composites)")
        if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("--composites runs on one GPU: --gpus > 1 is not supported for the composites (run the totals sharded, the "
                             "composites apart)")
        if args.ingest == "device" or args.device_ingest:
            raise SystemExit("--composites prepares the data on the host: --ingest device / --device-ingest is not supported for the "
                             "composites (--ingest auto resolves to host)")
    if getattr(args, "composite_sections", False):
        if args.fixed:
            raise SystemExit("--composite-sections goes with -t / -c: ONE fixed box has --sections, the sections on the box's own rows; a "
                             "system-relative section is laid on the box-relative rows of the boxes that follow a system")
        if args.trackfiles is not None:
            raise SystemExit("--composite-sections follows ONE system: --trackfiles analyses a batch of tracks and has no system-relative "
                             "sections (run -t --trackfile FILE --composite-sections for the track that matters)")
        if args.choose and (args.choose_systems is not None or args.choose_starts is not None):
            raise SystemExit("--composite-sections follows ONE system: -c --choose-systems / --choose-starts follows a batch and has no "
                             "system-relative sections (run -t --trackfile on a track it wrote, with --composite-sections)")
        if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("--composite-sections runs on one GPU: --gpus > 1 is not supported for the system-relative sections (their "
                             "time sums would have to merge in time order; run the totals sharded, the sections apart)")
    if getattr(args, "lon_sections", False):
        if not args.fixed:
            raise SystemExit("--lon-sections goes with -f/--fixed: a longitude-pressure section lies on the columns of ONE fixed box; the "
                             "boxes of a -t / -c run move, and have --composite-lon-sections on their box-relative columns")
        if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("--lon-sections runs on one GPU: --gpus > 1 is not supported for the longitude-pressure sections (run the "
                             "totals sharded, the sections apart)")
        if getattr(args, "wavenumbers_chunk", None) is not None:
            raise SystemExit("--lon-sections prepares the data on the host: --wavenumbers-chunk streams the series and is not supported for "
                             "the longitude-pressure sections (they read the field cubes once more)")
        if args.ingest == "device" or args.device_ingest:
            raise SystemExit("--lon-sections prepares the data on the host: --ingest device / --device-ingest is not supported for the "
                             "longitude-pressure sections (--ingest auto resolves to host)")
    if getattr(args, "composite_lon_sections", False):
        if args.fixed:
            raise SystemExit("--composite-lon-sections goes with -t / -c: ONE fixed box has --lon-sections, the sections on the box's own "
                             "columns; a system-relative section is laid on the box-relative columns of the boxes that follow a system")
        if args.trackfiles is not None:
            raise SystemExit("--composite-lon-sections follows ONE system: --trackfiles analyses a batch of tracks and has no system-relative "
                             "longitude-pressure sections (run -t --trackfile FILE --composite-lon-sections for the track that matters)")
        if args.choose and (args.choose_systems is not None or args.choose_starts is not None):
            raise SystemExit("--composite-lon-sections follows ONE system: -c --choose-systems / --choose-starts follows a batch and has no "
                             "system-relative longitude-pressure sections (run -t --trackfile on a track it wrote, with "
                             "--composite-lon-sections)")
        if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("--composite-lon-sections runs on one GPU: --gpus > 1 is not supported for the system-relative "
                             "longitude-pressure sections (run the totals sharded, the sections apart)")
        if args.ingest == "device" or args.device_ingest:
            raise SystemExit("--composite-lon-sections prepares the data on the host: --ingest device / --device-ingest is not supported for "
                             "the system-relative longitude-pressure sections (--ingest auto resolves to host)")
    n = getattr(args, "wavenumbers", None)
    chunk = getattr(args, "wavenumbers_chunk", None)
    if n is None:
        if chunk is not None:
            raise SystemExit("--wavenumbers-chunk goes with --wavenumbers N: it streams the series of the zonal-wavenumber spectra; "
                             "--device-ingest streams a plain -f / -t / -c run")
        if getattr(args, "wavenumbers_generation", False):
            raise SystemExit("--wavenumbers-generation goes with --wavenumbers N: Ge(n) is one more of the zonal-wavenumber spectra")
        if getattr(args, "wavenumbers_interactions", False):
            raise SystemExit("--wavenumbers-interactions goes with --wavenumbers N: S(n) and L(n) are two more of the zonal-wavenumber spectra")
        if getattr(args, "wavenumbers_budget", False):
            raise SystemExit("--wavenumbers-budget goes with --wavenumbers N: BAe(n), BKe(n) and the residuals are more of the zonal-wavenumber spectra")
        return
    from lorenzcycletoolkit_amd._lib import LEC_MAX_WAVENUMBERS
    if not (args.fixed and args.periodic):
        raise SystemExit("--wavenumbers goes with -f --periodic: a zonal-wavenumber spectrum exists on a full ring of longitudes only")
    if n < 1:
        raise SystemExit("--wavenumbers must be >= 1")
    if n > LEC_MAX_WAVENUMBERS:
        raise SystemExit(f"--wavenumbers must be <= {LEC_MAX_WAVENUMBERS} (LEC_MAX_WAVENUMBERS, include/lec_hip.h)")
    if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--wavenumbers runs on one GPU: --gpus > 1 is not supported for the spectra (run the totals sharded, the spectra apart)")
    if chunk is not None:
        if chunk < 1:
            raise SystemExit("--wavenumbers-chunk must be >= 1 time steps")
        if args.ingest == "host":
            raise SystemExit("--wavenumbers-chunk streams the file to the GPU, --ingest host prepares it on the host: give one of the two")
        return
    if args.ingest == "device" or args.device_ingest:
        raise SystemExit("--wavenumbers prepares the data on the host: --ingest device / --device-ingest is not supported for the spectra "
                         "(--ingest auto resolves to host; --wavenumbers-chunk N streams the series and computes the spectra chunk by chunk)")


def refuse_batch_chunk_options(args):
    """--batch-chunk is the streamed analysis of a batch of tracks; said before anything is created."""
    if args.batch_chunk is None:
        return
    many = args.choose and (args.choose_systems is not None or args.choose_starts is not None)
    if args.trackfiles is None and not many:
        raise SystemExit("--batch-chunk goes with --trackfiles (or -c --choose-systems / --choose-starts): it streams a batch of tracks; "
                         "--device-ingest streams a single -f / -t / -c run")
    if args.batch_chunk < 1:
        raise SystemExit("--batch-chunk must be >= 1 time steps")
    if args.ingest == "host":
        raise SystemExit("--batch-chunk streams the file to the GPU, --ingest host prepares it on the host: give one of the two")


def refuse_batch_composites_options(args):
    """--batch-composites is the composites of a batch of tracks held as union cubes on one GPU; said before anything is created."""
    clock = getattr(args, "batch_composites_phase", None)
    if clock is not None:
        if not getattr(args, "batch_composites", False):
            raise SystemExit("--batch-composites-phase bins the composites of a batch of tracks: it goes with --batch-composites")
        from lorenzcycletoolkit_amd.batch import parse_phase_clock
        try:
            parse_phase_clock(clock)
        except ValueError as e:
            raise SystemExit(str(e))
    if not getattr(args, "batch_composites", False):
        return
    many = args.choose and (args.choose_systems is not None or args.choose_starts is not None)
    if args.fixed:
        raise SystemExit("--batch-composites goes with -t --trackfiles or -c --choose-systems / --choose-starts: ONE fixed box has --maps, "
                         "the maps on the box's own points")
    if args.trackfiles is None and not many:
        raise SystemExit("--batch-composites composites a BATCH of tracks (-t --trackfiles, -c --choose-systems / --choose-starts): "
                         "ONE system has --composites (-t --trackfile FILE --composites, -c --composites)")
    if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--batch-composites runs on one GPU: --gpus > 1 is not supported for a batch of tracks")
    if args.batch_chunk is not None:
        raise SystemExit("--batch-composites reads the union cubes once more: --batch-chunk streams the batch and never holds them "
                         "(run the batch without --batch-chunk)")
    if args.ingest == "device" or args.device_ingest:
        raise SystemExit("--batch-composites prepares the data on the host: --ingest device / --device-ingest is not supported for the "
                         "batch composites (--ingest auto resolves to host)")


def _join_threshold(argv):
    """``--choose-threshold -5e-5`` as ``--choose-threshold=-5e-5`` (``--choose-end-threshold`` likewise): argparse takes a negative
    number in exponent form for an option."""
    out = list(argv)
    for n in range(len(out) - 1):
        if out[n] in ("--choose-threshold", "--choose-end-threshold"):
            try:
                float(out[n + 1])
            except ValueError:
                continue
            out[n: n + 2] = [f"{out[n]}={out[n + 1]}", None]
    return [x for x in out if x is not None]


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = create_arg_parser().parse_args(_join_threshold(argv))
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    refuse_choose_options(args)
    refuse_periodic_options(args)
    refuse_batch_chunk_options(args)
    refuse_batch_composites_options(args)
    refuse_series_options(args)
    if args.trackfiles is not None:
        return main_batch(args, argv)
    if args.choose and (args.choose_systems is not None or args.choose_starts is not None):
        return main_choose_batch(args, argv)
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        # this process only starts the ranks (before anything touches a GPU) and waits for them
        from lorenzcycletoolkit_amd.parallel import launch_local_ranks
        sys.exit(launch_local_ranks(__file__, argv, args.gpus))
    if env_world is not None and args.gpus > 1 and int(env_world) != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} contradicts WORLD_SIZE={env_world}")
    from lorenzcycletoolkit_amd.parallel import shard_from_env
    args.shard = shard_from_env()                      # None: the ordinary one-process run
    method = "fixed" if args.fixed else ("track" if args.track else "choose")
    tree_is_new = not os.path.isdir(os.path.join("./LEC_Results/", "".join(args.infile.split("/")[-1].split(".nc")) + "_" + method))
    if args.shard is None or args.shard.root:
        results_subdirectory, figures_directory, results_subdirectory_vertical_levels = setup_results_directory(args, method)
    else:                                              # the paths only: rank 0 creates the tree and writes every file
        results_subdirectory = os.path.join("./LEC_Results/", "".join(args.infile.split("/")[-1].split(".nc")) + "_" + method)
        results_subdirectory_vertical_levels = os.path.join(results_subdirectory, "results_vertical_levels")
        figures_directory = os.path.join(results_subdirectory, "Figures")
    app_logger = initialize_logging(results_subdirectory, args)
    if phases.enabled():             # (measurement runs only: brings the library load and the HIP context forward so that they show as a phase)
        import torch
        from lorenzcycletoolkit_amd import _lib
        _lib.load()
        torch.zeros(1, device=(args.shard.device if args.shard is not None else os.environ.get("LEC_DEVICE", "cuda:0")))
        torch.cuda.synchronize()
        phases.mark("library_and_hip_init")
    app_logger.info("Starting LEC analysis")
    app_logger.info(f"Command line arguments: {args}")
    if args.shard is not None:
        app_logger.info(f"Time-sharded run: {args.shard.world} ranks (backend {args.shard.backend}), one GPU each; rank 0 writes the results")
    try:
        if args.choose:
            # phase A: the 850-hPa slices -> lec_follow -> the track file; from here on the run IS -t on that track
            import copy
            from lorenzcycletoolkit_amd.follow import write_choose_track
            written = write_choose_track(args, results_subdirectory, app_logger, device=os.environ.get("LEC_DEVICE", "cuda:0"))
            phases.mark("choose_track")
            args = copy.copy(args)
            args.track, args.choose, args.trackfile, args.choose_track = True, False, written, written
        opened, auto_chose = None, False
        wave_chunk = getattr(args, "wavenumbers_chunk", None)
        if args.ingest == "device" or wave_chunk is not None:
            args.device_ingest = True
            if wave_chunk is not None:
                app_logger.info(f"--wavenumbers-chunk {wave_chunk}: the file is streamed to the GPU, {wave_chunk} time steps per pipeline slot, "
                                "and the spectra are computed chunk by chunk (lec_level_spec_ring: no assembled row records)")
        elif args.ingest == "auto" and getattr(args, "wavenumbers", None) is not None:
            app_logger.info("--wavenumbers: --ingest auto resolves to host (the spectra run on host-prepared cubes)")
        elif args.ingest == "auto" and getattr(args, "maps", False):
            app_logger.info("--maps: --ingest auto resolves to host (the maps read host-prepared cubes once more)")
        elif args.ingest == "auto" and getattr(args, "composites", False):
            app_logger.info("--composites: --ingest auto resolves to host (the composites read the host-prepared series once more)")
        elif args.ingest == "auto" and getattr(args, "lon_sections", False):
            app_logger.info("--lon-sections: --ingest auto resolves to host (the longitude-pressure sections read host-prepared cubes once more)")
        elif args.ingest == "auto" and getattr(args, "composite_lon_sections", False):
            app_logger.info("--composite-lon-sections: --ingest auto resolves to host (the sections read the host-prepared series once more)")
        elif args.ingest == "auto" and not args.device_ingest:
            from lorenzcycletoolkit_amd.ingest import prefers_device_ingest
            args.device_ingest, opened = prefers_device_ingest(args, "inputs/namelist", keep_open=True, app_logger=app_logger)
            auto_chose = args.device_ingest
            if args.device_ingest:
                app_logger.info("The input is a deflated NetCDF-4 file whose chunks the GPU can inflate, or a large file: streaming it to the "
                                "GPU (--ingest device); --ingest host prepares the data on the host instead (same results)")
        analyse = lambda d: run_lec_analysis(d, args, results_subdirectory, figures_directory, results_subdirectory_vertical_levels, app_logger)
        data = None
        if args.device_ingest:
            from lorenzcycletoolkit_amd.ingest import StreamedRefusal, prepare_streamed, refusals
            refused = None
            try:
                with refusals():
                    data = prepare_streamed(args, "inputs/namelist", app_logger, chunk_steps=wave_chunk, raw=opened)
                phases.mark("open_and_plan")
                try:
                    analyse(data)
                finally:
                    data.raw.close()
            except StreamedRefusal as e:
                # A streamed path that --ingest auto chose BY ITSELF must not fail a run the host preparation can do: the file is closed, the
                # reason logged, and the data are prepared on the host.  Only a REFUSAL of the streamed path counts (raised around
                # prepare_streamed / lec_streamed: before the engine has produced anything) -- an error later in the run (CSV writing,
                # plotting) is an error, not a reason to analyse everything a second time.  Asked for explicitly (--ingest device /
                # --device-ingest) the refusal stands.
                if not auto_chose or args.shard is not None:       # (ranks of a sharded run must not part ways)
                    raise e.__cause__ if e.__cause__ is not None else e
                refused = str(e)
            if refused is not None:
                # (outside the handler: the traceback -- and through its frames the failed attempt's device buffers -- is released first)
                if data is None and opened is not None:
                    opened.close()
                app_logger.warning(f"--ingest auto: the streamed path refused this input ({refused}); preparing the data on the host instead")
                args.device_ingest, data = False, None
                import gc
                import torch
                gc.collect()
                if torch.cuda.is_available():
                    torch.cuda.empty_cache()
        if not args.device_ingest:
            data = prepare_data(args, "inputs/namelist", app_logger)
            phases.mark("open_decode_and_prepare")
            analyse(data)
        if args.shard is not None:
            args.shard.barrier()                       # the ranks leave together, after rank 0 has written the files
    except Exception:
        app_logger.exception("LEC analysis failed")
        if tree_is_new and (args.shard is None or args.shard.root):
            _leave_only_the_log(results_subdirectory)
        raise
    finally:
        phases.mark("end")
        phases.dump({"argv": argv})
        if args.shard is not None:
            import torch.distributed as dist
            if dist.is_initialized():
                dist.destroy_process_group()


def refuse_batch_options(args):
    """What a --trackfiles run does not do, said before any GPU work."""
    if not args.track:
        raise SystemExit("--trackfiles goes with -t/--track")
    if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--trackfiles runs on one GPU: --gpus > 1 is not supported for a batch of tracks")
    if (args.ingest == "device" or args.device_ingest) and args.batch_chunk is None:
        raise SystemExit("--trackfiles prepares the data on the host: --ingest device / --device-ingest is not supported for a batch of tracks "
                         "(--batch-chunk N streams the batch to the GPU)")


def main_batch(args, argv):
    """-t --trackfiles: every track's tree as its own -t --trackfile run writes it, one pass over the data (lorenzcycletoolkit_amd/batch.py)."""
    from lorenzcycletoolkit_amd import batch
    refuse_batch_options(args)
    return run_batch(args, argv, "_track_batch", "batch of tracks", lambda batch_dir, app_logger: batch.expand_trackfiles(args.trackfiles))


def main_choose_batch(args, argv):
    """-c --choose-systems K / --choose-starts FILE: the GPU finds (or is told) the systems of the first time step and follows them all in
    one launch (follow.write_choose_tracks); from the written tracks on the run IS -t --trackfiles on them."""
    import copy
    from lorenzcycletoolkit_amd import batch

    def tracks(batch_dir, app_logger):
        from lorenzcycletoolkit_amd.follow import write_choose_tracks
        written = write_choose_tracks(args, batch_dir, app_logger, device=os.environ.get("LEC_DEVICE", "cuda:0"))
        phases.mark("choose_track")
        return batch.expand_trackfiles(written)

    args = copy.copy(args)
    args.track, args.choose = True, False
    return run_batch(args, argv, "_choose_batch", "several systems of -c", tracks)


def run_batch(args, argv, suffix, what, trackfiles_of):
    """The body of a run over many tracks: the log and batch.csv in LEC_Results/<stem><suffix>/, one tree per track.
    ``trackfiles_of(batch_dir, app_logger)`` gives the track files once the log is open (it may write them first)."""
    from lorenzcycletoolkit_amd import batch
    args.shard = None
    stem = "".join(args.infile.split("/")[-1].split(".nc"))
    batch_dir = os.path.join("./LEC_Results/", stem + suffix)
    created = [] if os.path.isdir(batch_dir) else [batch_dir]
    os.makedirs(batch_dir, exist_ok=True)
    app_logger = initialize_logging(batch_dir, args)
    app_logger.info(f"Starting LEC analysis ({what})")
    app_logger.info(f"Command line arguments: {args}")
    try:
        start_time = time.time()
        trackfiles = trackfiles_of(batch_dir, app_logger)
        variable_list_df = pd.read_csv("inputs/namelist", sep=";", index_col=0, header=0)
        # a track across the +-180 meridian takes the longitude axis 0..360 (dataset.track_lon_origin): the tracks are partitioned by
        # origin, each partition (at most two) is a pass of its own; a batch whose tracks are all origin 0 is the one pass it was
        parts = batch.partition_by_origin(args, trackfiles, "inputs/namelist", app_logger)
        if len(parts) > 1 or parts[0][0]:
            app_logger.info("Longitude axis per track: " + "; ".join(f"{'0..360 (across the +-180 meridian)' if origin else '-180..180'}: "
                            + ", ".join(trackfiles[n] for n in members) for origin, members in parts) + f" -- {len(parts)} pass(es) over the data")
        batch_composites = bool(getattr(args, "batch_composites", False))
        if batch_composites and len(parts) > 1:
            raise ValueError("--batch-composites: the tracks take two longitude axes (" + "; ".join(
                f"{'0..360' if origin else '-180..180'}: " + ", ".join(trackfiles[n] for n in members) for origin, members in parts)
                + "), which are two passes over the data with no common ensemble: run the two sets apart")
        if batch_composites and args.ingest == "auto":
            app_logger.info("--batch-composites: --ingest auto resolves to host (the composites read the host-prepared union cubes once more)")
        rows = [None] * len(trackfiles)
        told = False
        for origin, members in parts:
            raw = None
            if args.batch_chunk is not None:
                # the streamed batch: the file stays memory-mapped bytes, the plan is made on its coordinates; a file the streamed path
                # does not read is refused (the host union is what the flag exists to avoid)
                from lorenzcycletoolkit_amd import dataset as ds
                try:
                    raw = ds.open_raw(ds.series_paths(args), ds.read_namelist("inputs/namelist", app_logger), mpas=bool(getattr(args, "mpas", False)), app_logger=app_logger)
                except ValueError as e:
                    raise ValueError(f"--batch-chunk: the streamed path does not read this file ({e}); without --batch-chunk the batch is prepared on the host") from e
                if not told:
                    from lorenzcycletoolkit_amd.ingest import note_series_inflate
                    note_series_inflate(args, raw, app_logger)
                    told = True
                try:
                    plan = batch.plan_batch(raw.lat, raw.lon, raw.level, raw.time, raw.level_units, raw.names, [trackfiles[n] for n in members],
                                            app_logger, origin)
                except Exception:
                    raw.close()
                    raise
                phases.mark("open_and_plan")
            else:
                data, plan = batch.prepare_union(args, [trackfiles[n] for n in members], "inputs/namelist", app_logger, lon_origin=origin)
                phases.mark("open_decode_and_prepare")
            # --batch-composites: every track's shapes and axes, before a file is written; the box shapes are the ensembles
            shapes = batch.composites_check(plan) if batch_composites else None
            directories = []
            for tr in plan.tracks:
                tree = os.path.join("./LEC_Results/", f"{stem}_{tr.stem}_track")
                if not os.path.isdir(tree):
                    created.append(tree)
                vl, fig = os.path.join(tree, "results_vertical_levels"), os.path.join(tree, "Figures")
                for d in (fig, tree, vl):
                    os.makedirs(d, exist_ok=True)
                directories.append((tree, fig, vl))
            if raw is not None:
                from lorenzcycletoolkit_amd.ingest import StreamedRefusal
                try:
                    lec_moving_batch_streamed(raw, variable_list_df, plan, directories, app_logger, args)
                except StreamedRefusal as e:        # no fall-back to the host union: that is the path the flag exists to avoid
                    raise ValueError(f"--batch-chunk: the streamed path declines this input ({e}); without --batch-chunk the batch is prepared on the host") from e
                finally:
                    raw.close()
            else:
                lec_moving_batch(data, variable_list_df, plan, directories, app_logger, args, batch_dir=batch_dir, composite_shapes=shapes)
                del data
            for n, tr, d in zip(members, plan.tracks, directories):
                rows[n] = (tr.path, d[0], tr.n)
            del plan
        pd.DataFrame({"trackfile": [r[0] for r in rows], "results_directory": [r[1] for r in rows],
                      "steps": [r[2] for r in rows]}).to_csv(os.path.join(batch_dir, "batch.csv"), index=False)
        app_logger.info("Analysis complete! Moving framework ran %d tracks in %.2f seconds" % (len(rows), time.time() - start_time))
    except Exception:
        app_logger.exception("LEC analysis failed")
        for tree in created:
            _leave_only_the_log(tree)
            if tree != batch_dir and not os.listdir(tree):
                os.rmdir(tree)
        raise
    finally:
        phases.mark("end")
        phases.dump({"argv": argv})


if __name__ == "__main__":
    status = main(sys.argv[1:])
    # The results are on disk and the logs flushed: leave without the interpreter's teardown.  A run that pinned / registered tens of
    # GB of host memory and holds a HIP context spends 1-2.5 s there (freeing pinned blocks one by one, unloading the runtime) -- a
    # quarter of the wall clock of a 96-step ERA5 file (profiles/r04_notes.md section 6); the operating system reclaims it all at once.
    # Everything must be flushed BEFORE this line: os._exit skips atexit handlers and buffered file objects (phases.dump and the CSV
    # writers close their files; logging is shut down here).  main()'s return value is the exit status -- a failure raises and never
    # gets here, so the interpreter's ordinary exit reports it.
    logging.shutdown()
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(int(status or 0))

"""ctypes binding of include/blah2hip.h.

The HIP library is the product; there is no CPU fallback.  Importing this
module fails loudly when ``libblah2hip.so`` has not been built, and every call
raises :class:`Blah2HipError` on a non-zero status.
"""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libblah2hip.so")

OK = 0
ERR_INVALID, ERR_HIP, ERR_UNSUPPORTED, ERR_UNDERFLOW, ERR_NO_DEVICE, ERR_CAPACITY = -1, -2, -3, -4, -5, -6
FMT_C32, FMT_I16, FMT_F16, FMT_I16X_C32Y, FMT_I8, FMT_I8X_C32Y = 0, 1, 2, 3, 4, 5
K_RANGE, K_DOPPLER, K_METRICS, K_CFAR, K_SAT_ROWS, K_SAT_COLS, K_ROTATE, K_BEAM, K_COV, K_BEARING, K_COUNT = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
KERNEL_NAMES = {K_RANGE: "range", K_DOPPLER: "doppler", K_METRICS: "metrics", K_CFAR: "cfar",
                K_SAT_ROWS: "sat_rows", K_SAT_COLS: "sat_cols", K_ROTATE: "rotate", K_BEAM: "beam", K_COV: "cov",
                K_BEARING: "bearing"}
CK_CORR, CK_REDUCE, CK_SOLVE, CK_FIR, CK_COUNT = 0, 1, 2, 3, 4
NK_NCI, NK_TRACK_POWER, NK_TRACK_SUM, NK_COUNT = 0, 1, 2, 3
NCI_KERNEL_NAMES = {NK_NCI: "nci", NK_TRACK_POWER: "track_power", NK_TRACK_SUM: "track_sum"}
CLUTTER_KERNEL_NAMES = {CK_CORR: "clutter_corr", CK_REDUCE: "clutter_reduce", CK_SOLVE: "clutter_solve",
                        CK_FIR: "clutter_fir"}
OPT_DOPPLER_KERNEL, OPT_RANGE_GRID, OPT_RANGE_KERNEL, OPT_DOPPLER_GRID, OPT_FFT_LEN, OPT_CFAR2D_KERNEL = 1, 2, 3, 4, 5, 6
OPT_LEAK_COMPENSATION = 7
OPT_HOT_COLUMNS = 8
OPT_CFAR2D_SEG_ROWS, OPT_CFAR2D_GRID = 9, 10
OPT_MULTI_SURV_RANGE = 11
OPT_RANGE_WALK = 12
OPT_CFAR_LOOKS = 13
OPT_TAPER_SEG_ROWS = 14
MAX_TAPER_SIDE = 4
TAPER_NONE, TAPER_HANN, TAPER_HAMMING, TAPER_BLACKMAN, TAPER_BLACKMAN_HARRIS, TAPER_NUTTALL, TAPER_FLATTOP = 0, 1, 2, 3, 4, 5, 6
TAPER_KINDS = {"none": TAPER_NONE, "hann": TAPER_HANN, "hamming": TAPER_HAMMING, "blackman": TAPER_BLACKMAN,
               "blackmanharris": TAPER_BLACKMAN_HARRIS, "nuttall": TAPER_NUTTALL, "flattop": TAPER_FLATTOP}
MAX_CFAR_LOOKS = 1024
CFAR_GO, CFAR_SO = 1, 2  # kind of blah2hip_gocfar*: greatest-of, smallest-of
MAX_NCI_WINDOW = 16
WALK_AUTO, WALK_STATIC, WALK_TICKET = 0, 1, 2
MULTI_AUTO, MULTI_SHARED, MULTI_PER_CHANNEL = 0, 1, 2
MAX_SURV = 8
MAX_BEAMS = 8
MAX_BEARING_GRID = 384
BEARING_WRAP = 1
LEAK_OFF, LEAK_AUTO, LEAK_ALWAYS = 0, 1, 2
CFAR2D_AUTO, CFAR2D_TILE, CFAR2D_SAT, CFAR2D_STREAM = 0, 1, 2, 3
CLUTTER_OPT_SOLVE_K, CLUTTER_OPT_FFT_LEN, CLUTTER_OPT_CORR, CLUTTER_OPT_SOLVE_FORM, CLUTTER_OPT_SOLVE_E, CLUTTER_OPT_FIR_CARRY = 1, 2, 3, 4, 5, 6
CLUTTER_OPT_SOLVE_SPIN_LIMIT = 7
CLUTTER_OPT_CORR_GRID = 8
CLUTTER_SOLVE_AUTO, CLUTTER_SOLVE_STEPWISE, CLUTTER_SOLVE_LOOKAHEAD = 0, 1, 2
CLUTTER_INFO_SOLVE_FORM, CLUTTER_INFO_SOLVE_E, CLUTTER_INFO_SOLVE_G, CLUTTER_INFO_SOLVE_FAULT, CLUTTER_INFO_SOLVE_RETRIES = 1, 2, 3, 4, 5
CLUTTER_INFO_CORR_FORM, CLUTTER_INFO_FIR_CARRY, CLUTTER_INFO_CHUNKS, CLUTTER_INFO_BLOCKS = 6, 7, 8, 9
CLUTTER_INFO_CORR_GRID = 10
CLUTTER_CORR_AUTO, CLUTTER_CORR_HALF, CLUTTER_CORR_WINDOW, CLUTTER_CORR_DIRECT = 0, 1, 2, 3
DOP_AUTO, DOP_TILE8, DOP_TILE16, DOP_TILEM, DOP_COLUMN, DOP_DIRECT, DOP_TILEW, DOP_TILEW2, DOP_TILE16WG, DOP_SUB4, DOP_TILE8K, DOP_TILEW4 = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11
DOP_PFA513 = 12
DOPPLER_KERNEL_NAMES = {DOP_AUTO: "auto", DOP_TILE8: "tile8", DOP_TILE16: "tile16", DOP_TILEM: "tilem",
                        DOP_COLUMN: "column", DOP_DIRECT: "direct", DOP_TILEW: "tilew", DOP_TILEW2: "tilew2", DOP_TILE16WG: "tile16wg", DOP_SUB4: "sub4", DOP_TILE8K: "tile8k", DOP_TILEW4: "tilew4",
                        DOP_PFA513: "pfa513"}
RANGE_E16, RANGE_E8, RANGE_WAVE, RANGE_WAVE1K, RANGE_PS, RANGE_FIR = 1, 2, 3, 5, 6, 7
RANGE_SHARED = 8
INFO_LAST_DOPPLER_KERNEL, INFO_LAST_RANGE_KERNEL, INFO_DOPPLER_FFT_LEN, INFO_RANGE_GRID, INFO_NUM_CU = 1, 2, 3, 4, 5
INFO_DOPPLER_GRID, INFO_DOPPLER_TILES = 6, 7
INFO_LEAK_LAGS, INFO_LEAK_MAX_E12 = 8, 9
INFO_HOT_COLUMNS, INFO_HOT_COLUMNS_MISSED = 10, 11
INFO_CFAR2D_SEG_ROWS, INFO_CFAR2D_GRID = 12, 13
INFO_DETECT_GRID, INFO_DETECT_TILED = 14, 15
INFO_BEARING_GRID = 16
INFO_TAPER_GRID = 17
INFO_MIGRATE_GRID = 18
MAX_MIGRATION = 512
INFO_RATE_GRID = 19
MAX_RATES = 16
INFO_TRACK_GRID, INFO_TRACK_MAX_SHIFT = 20, 21
MAX_TRACK_SHIFT = 1048576
INFO_CARRIER_GRID = 22
MAX_CARRIERS = 8
CARRIER_NEAREST, CARRIER_LINEAR = 0, 1
CARRIER_INTERPS = {"nearest": CARRIER_NEAREST, "linear": CARRIER_LINEAR}
MAX_CMAP_MEMORY = 64
CMAP_NORMALISE = 1
MAX_ATOMS = 32
CLEAN_OPT_GRAM_GRID = 1
CLEAN_INFO_GRAM_GRID, CLEAN_INFO_SUBTRACT_GRID = 1, 2
CLK_ATOMS, CLK_GRAM, CLK_FOLD, CLK_SOLVE, CLK_SUBTRACT, CLK_COUNT = 0, 1, 2, 3, 4, 5
CLEAN_KERNEL_NAMES = {CLK_ATOMS: "clean_atoms", CLK_GRAM: "clean_gram", CLK_FOLD: "clean_fold", CLK_SOLVE: "clean_solve",
                      CLK_SUBTRACT: "clean_subtract"}
MAX_DDC_CARRIERS, MAX_DDC_DECIM, MAX_DDC_TAPS = 8, 64, 1024
DDC_INFO_TILE, DDC_INFO_NEXT_SAMPLE = 1, 2
DK_DDC, DK_TAIL, DK_COUNT = 0, 1, 2
DDC_KERNEL_NAMES = {DK_DDC: "ddc", DK_TAIL: "ddc_tail"}


class Blah2HipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"blah2hip error {code}: {msg}")
        self.code = code


class AmbDims(C.Structure):
    _fields_ = [("n_doppler_bins", C.c_uint32), ("n_delay_bins", C.c_uint32), ("n_corr", C.c_uint32),
                ("nfft", C.c_uint32), ("n_samples", C.c_uint32), ("n_used", C.c_uint32),
                ("cpi", C.c_double), ("doppler_middle", C.c_double), ("fft_len", C.c_uint32),
                ("n_seg", C.c_uint32), ("seg_len", C.c_uint32), ("max_batch", C.c_uint32)]


class Hit(C.Structure):
    _fields_ = [("row", C.c_int32), ("col", C.c_int32), ("snr", C.c_double)]


class Det(C.Structure):
    _fields_ = [("row", C.c_int32), ("col", C.c_int32), ("delay", C.c_double), ("doppler", C.c_double), ("snr", C.c_double)]


class Atom(C.Structure):
    _fields_ = [("delay", C.c_int32), ("reserved", C.c_int32), ("doppler", C.c_double)]


class Bearing(C.Structure):
    _fields_ = [("index", C.c_int32), ("adaptive", C.c_int32), ("offset", C.c_double), ("power", C.c_double), ("coherence", C.c_double)]


# every symbol include/blah2hip.h declares: name -> (restype, argtypes)
_vp, _u32, _i32, _dbl = C.c_void_p, C.c_uint32, C.c_int32, C.c_double
SYMBOLS = {
    "blah2hip_last_error": (C.c_char_p, []),
    "blah2hip_version": (C.c_char_p, []),
    "blah2hip_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "blah2hip_next_hamming": (_u32, [_u32]),
    "blah2hip_amb_create": (C.c_int, [_i32, _i32, _i32, _i32, _u32, _u32, C.c_int, C.c_int, _u32, C.POINTER(_vp)]),
    "blah2hip_amb_create_ex": (C.c_int, [_i32, _i32, _i32, _i32, _u32, _u32, C.c_int, _u32, C.c_int, _u32, C.POINTER(_vp)]),
    "blah2hip_amb_destroy": (C.c_int, [_vp]),
    "blah2hip_amb_get_dims": (C.c_int, [_vp, C.POINTER(AmbDims)]),
    "blah2hip_amb_get_axes": (C.c_int, [_vp, _vp, _vp]),
    "blah2hip_amb_set_option": (C.c_int, [_vp, C.c_int, C.c_int64]),
    "blah2hip_amb_get_info": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int64)]),
    "blah2hip_amb_process_c64": (C.c_int, [_vp, _vp, _vp, _u32, _vp, _vp]),
    "blah2hip_amb_process_c32": (C.c_int, [_vp, _vp, _vp, _u32, _vp, _vp]),
    "blah2hip_amb_process_i16": (C.c_int, [_vp, _vp, _u32, _vp, _vp]),
    "blah2hip_amb_process_i8": (C.c_int, [_vp, _vp, _vp, _u32, _vp, _vp]),
    "blah2hip_amb_process_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _u32, C.c_uint64, _vp, _vp, _vp]),
    "blah2hip_amb_process_multi_dev": (C.c_int, [_vp, C.c_int, _vp, C.POINTER(_vp), _u32, _u32, C.c_uint64, _vp, _vp, _vp]),
    "blah2hip_amb_process_multi_c32": (C.c_int, [_vp, _vp, C.POINTER(_vp), _u32, _u32, _vp, _vp]),
    "blah2hip_amb_read_last": (C.c_int, [_vp, _u32, _vp, _vp]),
    "blah2hip_amb_db_dev": (C.c_int, [_vp, _vp, _vp, _u32, _vp, _vp]),
    "blah2hip_amb_beamform_dev": (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp, _vp, _vp]),
    "blah2hip_amb_beamform_wdev": (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp, _vp, _vp]),
    "blah2hip_amb_covariance_dev": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp]),
    "blah2hip_amb_mvdr_weights_dev": (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _dbl, _vp, _vp, _vp]),
    "blah2hip_amb_sample_covariance_dev": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), _u32, _u32, C.c_uint64, _u32, _u32, _vp, _vp]),
    "blah2hip_amb_beam_samples_dev": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), _u32, _u32, C.c_uint64, _vp, _u32, C.POINTER(_vp), C.c_uint64, _vp]),
    "blah2hip_amb_beam_samples_wdev": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), _u32, _u32, C.c_uint64, _vp, _u32, C.POINTER(_vp), C.c_uint64, _vp]),
    "blah2hip_amb_snapshot_dev": (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp]),
    "blah2hip_amb_bearing_dev": (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _dbl, _vp, _u32, _u32, _vp, _vp]),
    "blah2hip_nci_create": (C.c_int, [_vp, _u32, _u32, _u32, C.POINTER(_vp)]),
    "blah2hip_nci_destroy": (C.c_int, [_vp]),
    "blah2hip_nci_reset": (C.c_int, [_vp]),
    "blah2hip_nci_count": (C.c_int, [_vp, _u32, C.POINTER(_u32), C.POINTER(C.c_uint64)]),
    "blah2hip_nci_process_dev": (C.c_int, [_vp, _vp, _u32, _vp, _vp, _vp, _u32, C.POINTER(_u32), C.POINTER(C.c_uint64), _vp]),
    "blah2hip_nci_walk_table": (C.c_int, [_vp, _dbl, _dbl, _vp]),
    "blah2hip_nci_set_tracks": (C.c_int, [_vp, _vp, _vp, _u32, _u32]),
    "blah2hip_nci_process_tracks_dev": (C.c_int, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _u32, C.POINTER(_u32), C.POINTER(C.c_uint64), _vp]),
    "blah2hip_nci_set_timing": (C.c_int, [_vp, C.c_int]),
    "blah2hip_nci_get_timing": (C.c_int, [_vp, _vp, _vp]),
    "blah2hip_doppler_taper": (C.c_int, [C.c_int, C.c_int, _vp, C.POINTER(_u32)]),
    "blah2hip_amb_taper_dev": (C.c_int, [_vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp]),
    "blah2hip_migration_table": (C.c_int, [_vp, _dbl, _vp]),
    "blah2hip_amb_set_migration": (C.c_int, [_vp, _vp]),
    "blah2hip_amb_migrate_dev": (C.c_int, [_vp, _vp, _u32, _vp, _vp, _vp]),
    "blah2hip_doppler_rate": (C.c_int, [_vp, _dbl, _dbl, C.POINTER(_dbl)]),
    "blah2hip_amb_set_rates": (C.c_int, [_vp, _vp, _u32]),
    "blah2hip_amb_rate_bank_dev": (C.c_int, [_vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "blah2hip_carrier_table": (C.c_int, [_vp, _vp, _u32, C.c_int, _vp, _vp, _vp, _vp]),
    "blah2hip_amb_set_carriers": (C.c_int, [_vp, _vp, _u32, C.c_int]),
    "blah2hip_amb_fuse_carriers_dev": (C.c_int, [_vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "blah2hip_cfar_alpha": (C.c_int, [_dbl, _u32, _u32, _vp]),
    "blah2hip_cfar1d_dev": (C.c_int, [_vp, _vp, _vp, _u32, _dbl, _i32, _i32, _i32, _dbl, _vp, _u32, _vp, _vp]),
    "blah2hip_cfar1d_prepare": (C.c_int, [_vp, _dbl, _i32]),
    "blah2hip_cfar2d_prepare": (C.c_int, [_vp, _dbl, _i32, _i32, _i32, _i32]),
    "blah2hip_cfar1d_process": (C.c_int, [_vp, _u32, _dbl, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _u32, C.POINTER(_u32)]),
    "blah2hip_cfar1d_map": (C.c_int, [_vp, _u32, _u32, _vp, _vp, _dbl, _dbl, _i32, _i32, _i32, _dbl, C.c_int, _vp, _vp, _vp, _u32,
                                      C.POINTER(_u32)]),
    "blah2hip_cfar2d_dev": (C.c_int, [_vp, _vp, _vp, _u32, _dbl, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _u32, _vp, _vp]),
    "blah2hip_cfar2d_process": (C.c_int, [_vp, _u32, _dbl, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _u32,
                                          C.POINTER(_u32)]),
    "blah2hip_gocfar_alpha": (C.c_int, [_dbl, _u32, _u32, _vp, _vp, _vp]),
    "blah2hip_gocfar1d_dev": (C.c_int, [_vp, _vp, _vp, _u32, _dbl, _u32, _i32, _i32, _i32, _dbl, _vp, _u32, _vp, _vp]),
    "blah2hip_gocfar1d_prepare": (C.c_int, [_vp, _dbl, _u32, _i32, _i32]),
    "blah2hip_gocfar1d_process": (C.c_int, [_vp, _u32, _dbl, _u32, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _u32, C.POINTER(_u32)]),
    "blah2hip_gocfar2d_dev": (C.c_int, [_vp, _vp, _vp, _u32, _dbl, _u32, _i32, _i32, _i32, _i32, _dbl, _vp, _u32, _vp, _vp]),
    "blah2hip_gocfar2d_prepare": (C.c_int, [_vp, _dbl, _u32, _i32, _i32, _i32]),
    "blah2hip_gocfar2d_process": (C.c_int, [_vp, _u32, _dbl, _u32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _u32,
                                            C.POINTER(_u32)]),
    "blah2hip_oscfar_alpha": (C.c_int, [_dbl, _u32, _u32, _u32, _vp, _vp]),
    "blah2hip_oscfar1d_dev": (C.c_int, [_vp, _vp, _vp, _u32, _dbl, _u32, _i32, _i32, _i32, _dbl, _vp, _u32, _vp, _vp]),
    "blah2hip_oscfar1d_prepare": (C.c_int, [_vp, _dbl, _u32, _i32]),
    "blah2hip_oscfar1d_process": (C.c_int, [_vp, _u32, _dbl, _u32, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _u32, C.POINTER(_u32)]),
    "blah2hip_oscfar2d_dev": (C.c_int, [_vp, _vp, _vp, _u32, _dbl, _u32, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _u32, _vp, _vp]),
    "blah2hip_oscfar2d_prepare": (C.c_int, [_vp, _dbl, _u32, _i32, _i32, _i32, _i32]),
    "blah2hip_oscfar2d_process": (C.c_int, [_vp, _u32, _dbl, _u32, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _u32,
                                            C.POINTER(_u32)]),
    "blah2hip_cmap_alpha": (C.c_int, [_dbl, _u32, _u32, _vp]),
    "blah2hip_cmap_create": (C.c_int, [_vp, _u32, _u32, C.POINTER(_vp)]),
    "blah2hip_cmap_destroy": (C.c_int, [_vp]),
    "blah2hip_cmap_reset": (C.c_int, [_vp]),
    "blah2hip_cmap_age": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "blah2hip_cmap_prepare": (C.c_int, [_vp, _dbl]),
    "blah2hip_cmap_process_dev": (C.c_int, [_vp, _vp, _vp, _u32, _dbl, _i32, _dbl, _vp, _u32, _vp, _vp, _vp, _vp]),
    "blah2hip_cmap_gate_dev": (C.c_int, [_vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "blah2hip_cmap_read_background": (C.c_int, [_vp, _vp]),
    "blah2hip_clean_create": (C.c_int, [_u32, _dbl, _i32, _i32, C.c_int, _u32, C.POINTER(_vp)]),
    "blah2hip_clean_destroy": (C.c_int, [_vp]),
    "blah2hip_clean_set_option": (C.c_int, [_vp, C.c_int, C.c_int64]),
    "blah2hip_clean_get_info": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int64)]),
    "blah2hip_clean_atoms_dev": (C.c_int, [_vp, _vp, _vp, _u32, _vp, _u32, _dbl, _u32, _i32, _i32, _vp, _u32, _vp, _vp, _vp]),
    "blah2hip_clean_fit_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _u32, C.c_uint64, _vp, _u32, _vp, _dbl, _vp, _vp, _vp]),
    "blah2hip_clean_subtract_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _u32, C.c_uint64, _vp, _u32, _vp, _vp, _vp, _vp, C.c_uint64, _vp]),
    "blah2hip_clean_process_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _u32, C.c_uint64, _vp, _u32, _vp, _dbl, _vp, _vp, _vp, C.c_uint64, _vp]),
    "blah2hip_clean_read_last": (C.c_int, [_vp, _u32, _vp, _vp, _vp, _vp]),
    "blah2hip_clean_set_timing": (C.c_int, [_vp, C.c_int]),
    "blah2hip_clean_get_timing": (C.c_int, [_vp, _vp, _vp]),
    "blah2hip_ddc_design": (C.c_int, [_u32, _u32, _dbl, _dbl, _vp]),
    "blah2hip_ddc_create": (C.c_int, [_dbl, _u32, _vp, _u32, _vp, _u32, _u32, _u32, C.c_int, C.POINTER(_vp)]),
    "blah2hip_ddc_destroy": (C.c_int, [_vp]),
    "blah2hip_ddc_reset": (C.c_int, [_vp, C.c_uint64, _vp]),
    "blah2hip_ddc_process_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _u32, _u32, C.c_uint64, _vp, _vp, C.c_uint64, C.c_uint64, _vp]),
    "blah2hip_ddc_read_taps": (C.c_int, [_vp, _u32, _vp]),
    "blah2hip_ddc_get_info": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int64)]),
    "blah2hip_ddc_set_timing": (C.c_int, [_vp, C.c_int]),
    "blah2hip_ddc_get_timing": (C.c_int, [_vp, _vp, _vp]),
    "blah2hip_centroid": (C.c_int, [_vp, _vp, _vp, _u32, C.c_uint16, C.c_uint16, _dbl, _vp, _vp, _vp, C.POINTER(_u32)]),
    "blah2hip_interpolate": (C.c_int, [_vp, _vp, _vp, _u32, _vp, _u32, _u32, _vp, _vp, _dbl, C.c_int, C.c_int,
                                       _vp, _vp, _vp, C.POINTER(_u32)]),
    "blah2hip_detect_dev": (C.c_int, [_vp, _vp, _vp, _u32, _vp, _u32, _vp, C.c_uint16, C.c_uint16, _dbl, C.c_int, C.c_int, C.c_int,
                                      _vp, _u32, _vp, _vp]),
    "blah2hip_clutter_create": (C.c_int, [_i32, _i32, _u32, C.c_int, _u32, C.POINTER(_vp)]),
    "blah2hip_clutter_create_ex": (C.c_int, [_i32, _i32, _u32, _u32, C.c_int, _u32, C.POINTER(_vp)]),
    "blah2hip_clutter_destroy": (C.c_int, [_vp]),
    "blah2hip_clutter_process_c64": (C.c_int, [_vp, _vp, _vp, _u32, _vp, C.POINTER(C.c_int)]),
    "blah2hip_clutter_process_c32": (C.c_int, [_vp, _vp, _vp, _u32, _vp, C.POINTER(C.c_int)]),
    "blah2hip_clutter_process_dev": (C.c_int, [_vp, _vp, _vp, _u32, C.c_uint64, _vp, _vp, _vp]),
    "blah2hip_clutter_process_dev_fmt": (C.c_int, [_vp, C.c_int, _vp, _vp, _u32, C.c_uint64, _vp, C.c_uint64, _vp, _vp]),
    "blah2hip_clutter_process_multi_dev_fmt": (C.c_int, [_vp, C.c_int, _vp, C.POINTER(_vp), _u32, _u32, C.c_uint64, C.POINTER(_vp), C.c_uint64, _vp, _vp]),
    "blah2hip_clutter_set_option": (C.c_int, [_vp, C.c_int, C.c_int64]),
    "blah2hip_clutter_solve": (C.c_int, [_vp, _vp, _u32, _vp, _vp]),
    "blah2hip_clutter_solve_dev": (C.c_int, [_vp, _vp, _u32, _vp, _vp, _vp]),
    "blah2hip_clutter_get_info": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int64)]),
    "blah2hip_clutter_get_dims": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "blah2hip_clutter_read_last": (C.c_int, [_vp, _u32, _vp, _vp, C.POINTER(C.c_int)]),
    "blah2hip_clutter_set_timing": (C.c_int, [_vp, C.c_int]),
    "blah2hip_clutter_get_timing": (C.c_int, [_vp, _vp, _vp]),
    "blah2hip_spectrum_create": (C.c_int, [_u32, C.c_double, C.c_int, _u32, C.POINTER(_vp)]),
    "blah2hip_spectrum_destroy": (C.c_int, [_vp]),
    "blah2hip_spectrum_get_dims": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_uint64)]),
    "blah2hip_spectrum_process_c64": (C.c_int, [_vp, _vp, _u32, _vp]),
    "blah2hip_spectrum_process_c32": (C.c_int, [_vp, _vp, _u32, _vp]),
    "blah2hip_spectrum_process_dev": (C.c_int, [_vp, C.c_int, _vp, _u32, C.c_uint64, _vp, _vp]),
    "blah2hip_ctx_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "blah2hip_ctx_destroy": (C.c_int, [_vp]),
    "blah2hip_ctx_stream": (_vp, [_vp]),
    "blah2hip_ctx_sync": (C.c_int, [_vp]),
    "blah2hip_ctx_malloc": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "blah2hip_ctx_free": (C.c_int, [_vp, _vp]),
    "blah2hip_ctx_malloc_host": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "blah2hip_ctx_free_host": (C.c_int, [_vp, _vp]),
    "blah2hip_ctx_h2d": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "blah2hip_ctx_d2h": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "blah2hip_ctx_d2d": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "blah2hip_stream_read_dev": (C.c_int, [_vp, C.c_size_t, _vp, _vp]),
    "blah2hip_deblock_c32_dev": (C.c_int, [_vp, _u32, C.c_uint64, _u32, _u32, _vp, _vp, C.c_uint64, _vp]),
    "blah2hip_clutter_estimate_dev_fmt": (C.c_int, [_vp, C.c_int, _vp, _vp, _u32, C.c_uint64, _vp, _vp]),
    "blah2hip_clutter_taps_dev": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_u32), C.POINTER(_i32)]),
    "blah2hip_amb_set_fir": (C.c_int, [_vp, _vp, _u32, _i32]),
    "blah2hip_amb_fir_fusable": (C.c_int, [_vp, C.c_int, _u32, _i32]),
    "blah2hip_amb_result_ptrs": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "blah2hip_amb_set_timing": (C.c_int, [_vp, C.c_int]),
    "blah2hip_amb_get_timing": (C.c_int, [_vp, _vp, _vp]),
}

_lib = None


def load():
    """Loads libblah2hip.so (built by ``python -m blah2_amd.build``) or raises."""
    global _lib
    if _lib is not None:
        return _lib
    # BLAH2HIP_LIBRARY: another BUILD of the same HIP library (tools/ A/B runs of compile-time variants)
    path = os.environ.get("BLAH2HIP_LIBRARY", LIB_PATH)
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -m blah2_amd.build` "
            "(there is no CPU fallback for the HIP path)")
    # The PyTorch-ROCm wheel bundles its own libamdhip64/libhsa-runtime64.  Two HIP
    # runtimes in one process cannot both own the device, so when torch is installed
    # it is imported FIRST: libblah2hip.so's libamdhip64.so.7 dependency then binds
    # to the runtime torch already loaded (torch is only used by the Python harness
    # for device buffers/streams; C++ callers link /opt/rocm's runtime directly).
    if os.environ.get("BLAH2HIP_NO_TORCH_PRELOAD", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError when the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc):
    if rc != OK:
        raise Blah2HipError(rc, load().blah2hip_last_error().decode("utf-8", "replace"))


def device_count() -> int:
    n = C.c_int(0)
    rc = load().blah2hip_device_count(C.byref(n))
    return n.value if rc == OK else 0

"""blah2_amd -- MI355X (gfx950) cross-ambiguity engine for the blah2 passive radar.

Product code: ``csrc/`` (hand-written HIP kernels + the C ABI of
``include/blah2hip.h``), ``host/`` (C++ classes with the reference's own
surface) and the thin Python mirror in :mod:`blah2_amd.process`.  There is no
CPU implementation in this package: without ``libblah2hip.so`` and a GPU the
calls fail loudly.
"""
from ._lib import Blah2HipError, FMT_C32, FMT_F16, FMT_I16, FMT_I16X_C32Y, FMT_I8, FMT_I8X_C32Y, device_count, load  # noqa: F401
from .process import BEARING_DTYPE, DET_DTYPE, HIT_DTYPE, DetectionFinisher, deblock_c32_dev, dets_to_detection, hits_to_detection  # noqa: F401
from .process import Ambiguity, Centroid, CfarDetector1D, CfarDetector2D, Detection, Interpolate, Map, SpectrumAnalyser, WienerHopf, next_hamming, mvdr_weights, ula_steering, ula_weights, bearing, bearing_degrees, uca_steering, sample_covariance, beam_samples  # noqa: F401
from .process import MapIntegrator, cfar_alpha, cfar_alpha_table, cfar_pfa, integrate_ends, integrate_maps  # noqa: F401
from .process import (GoCfarDetector1D, GoCfarDetector2D, gocfar_alpha, gocfar_alpha_table, gocfar_counts,  # noqa: F401
                      gocfar_hits, gocfar_pfa, gocfar_table_for)
from .process import OsCfarDetector1D, OsCfarDetector2D, oscfar_alpha, oscfar_alpha_table, oscfar_hits, oscfar_pfa, oscfar_rank  # noqa: F401
from .process import doppler_taper, doppler_taper_f32, doppler_window, taper_gains, taper_maps  # noqa: F401
from .process import migrate_maps, migration_shifts, migration_table, range_map  # noqa: F401
from .process import doppler_rate, rate_bank, rate_bank_maps, rate_chirps  # noqa: F401
from .process import integrate_tracks, nci_walk_table, track_tables  # noqa: F401
from .process import ClutterMapDetector, clutter_map, clutter_map_alpha, clutter_map_alpha_table, clutter_map_pfa, clutter_map_weights, gate_hits  # noqa: F401
from .process import ATOM_DTYPE, EchoCanceller, clean_atoms, clean_fit, clean_replicas, clean_subtract, merge_clean_detections  # noqa: F401
from .process import Channelizer, ddc, ddc_design, ddc_taps  # noqa: F401
from .process import carrier_ratios, carrier_table, fuse_carriers  # noqa: F401

__all__ =["Ambiguity", "Centroid", "Interpolate", "CfarDetector1D", "CfarDetector2D", "Detection", "Map", "WienerHopf", "SpectrumAnalyser", "next_hamming", "Blah2HipError",
           "FMT_C32", "FMT_I16", "FMT_F16", "FMT_I16X_C32Y", "FMT_I8", "FMT_I8X_C32Y", "deblock_c32_dev", "device_count", "load",
           "DetectionFinisher", "dets_to_detection", "DET_DTYPE", "BEARING_DTYPE", "bearing", "bearing_degrees", "uca_steering"]

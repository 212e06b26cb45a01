/* blah2hip.h -- C ABI of the MI355X (gfx950) cross-ambiguity engine for blah2.
 *
 * The reference (30hours/blah2) has no plugin/FFI layer: the boundary of its
 * hot path is the C++ class surface that src/blah2.cpp constructs and calls
 * once per CPI on its processing thread (blah2.cpp:154-177, 263-289):
 *
 *   Ambiguity(delayMin,delayMax,dopplerMin,dopplerMax,fs,n,roundHamming)
 *       src/process/ambiguity/Ambiguity.h:34   ctor   Ambiguity.cpp:11-82
 *   Map<complex<double>>* Ambiguity::process(IqData* x, IqData* y)
 *       src/process/ambiguity/Ambiguity.h:44          Ambiguity.cpp:92-172
 *   void Map::set_metrics()                            src/data/Map.cpp:187-206
 *   CfarDetector1D(pfa,nGuard,nTrain,minDelay,minDoppler)::process(Map*)
 *       src/process/detection/CfarDetector1D.h:46,55   CfarDetector1D.cpp:23-100
 *   WienerHopf(delayMin,delayMax,nSamples)::process(IqData* x, IqData* y) -> bool
 *       src/process/clutter/WienerHopf.h:68,78         WienerHopf.cpp:58-163
 *
 * This header is what a binding for that path binds: opaque handles, plain
 * pointers and sizes, int status returns, no exceptions, no C++ or torch types.
 * blah2_amd/host/ holds source-compatible C++ classes (same names, arguments
 * and error behaviour as the reference's) implemented on top of it, and
 * INTEGRATION.md shows how they replace the FFTW path in blah2.cpp.
 *
 * Conventions
 *   - every function returns BLAH2HIP_OK (0) or a negative error code;
 *     blah2hip_last_error() returns a thread-local description of the last one.
 *   - "host" entry points take caller-owned host buffers, run on the handle's
 *     own stream and return when the results are in the output buffers.
 *   - "dev" entry points take device pointers that are already resident in HBM
 *     and a hipStream_t (as void*); they only enqueue work and never
 *     synchronise.  This is the chain the benchmark times.  Everything a dev
 *     call needs is allocated at *_create; the two exceptions are named where
 *     they occur (blah2hip_cfar1d_prepare / blah2hip_cfar2d_prepare: a threshold
 *     table per parameter tuple and the 2-D detector's summed-area table, built
 *     by the first call that needs them or ahead of time by *_prepare).
 *   - a handle is not re-entrant: one thread at a time, like the reference's
 *     objects (all three process() calls run on blah2.cpp's single t2 thread).
 *   - maps are complex fp32, interleaved (re,im), row-major [doppler][delay],
 *     the layout of Map<T>::data (src/data/Map.h:27).
 */
#ifndef BLAH2HIP_H
#define BLAH2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLAH2HIP_OK 0
#define BLAH2HIP_ERR_INVALID (-1)     /* bad argument */
#define BLAH2HIP_ERR_HIP (-2)         /* a HIP runtime call failed */
#define BLAH2HIP_ERR_UNSUPPORTED (-3) /* configuration outside what the kernels cover */
#define BLAH2HIP_ERR_UNDERFLOW (-4)   /* fewer samples than one CPI (IqData::pop_front throws, IqData.cpp:57-59) */
#define BLAH2HIP_ERR_NO_DEVICE (-5)   /* no gfx950 device visible */
#define BLAH2HIP_ERR_CAPACITY (-6)    /* output capacity too small */

/* input sample formats of the dev entry points */
#define BLAH2HIP_FMT_C32 0 /* two planes of complex fp32: x = reference, y = surveillance */
#define BLAH2HIP_FMT_I16 1 /* one buffer, int16 I1 Q1 I2 Q2 per sample (.rspduo, RspDuo.cpp:512-526) */
#define BLAH2HIP_FMT_F16 2 /* two planes of (re,im) IEEE half pairs; widened to fp32 on load, fp32 accumulate */
#define BLAH2HIP_FMT_I16X_C32Y 3 /* reference channel from the .rspduo buffer (tuner 1 of I1 Q1 I2 Q2), surveillance channel from a
                                  * complex fp32 plane: the ambiguity stage behind blah2hip_clutter_process_dev_fmt(FMT_I16), which
                                  * leaves x untouched and writes the filtered y as fp32 (WienerHopf.cpp:156-160) */
#define BLAH2HIP_FMT_I8 4 /* two planes of int8 (I, Q) pairs, 2 bytes per sample: d_x = reference, d_y = surveillance; CPI c at
                           * c * cpi_stride samples.  The sample format of the 8-bit receivers: the HackRF and the KrakenSDR /
                           * RTL-SDR callbacks (HackRf.cpp:119-127, Kraken.cpp:100-108) read each device's stream as int8_t, I
                           * then Q.  The bytes are taken as SIGNED, as both callbacks take them; RTL-SDR bytes are unsigned
                           * (offset binary) on the wire and the reference reinterprets them, so this format does too.  A
                           * plane needs 2-byte alignment only. */
#define BLAH2HIP_FMT_I8X_C32Y 5 /* reference channel from the int8 plane d_x, surveillance channel from a complex fp32 plane d_y:
                                 * the ambiguity stage behind blah2hip_clutter_process_dev_fmt(FMT_I8), the role FMT_I16X_C32Y has
                                 * for the .rspduo words (WienerHopf.cpp:156-160: x untouched, filtered y written as fp32) */

typedef struct blah2hip_amb_s *blah2hip_amb_t;
typedef struct blah2hip_clutter_s *blah2hip_clutter_t;
typedef struct blah2hip_spectrum_s *blah2hip_spectrum_t;

/* Derived sizes: the first block reproduces the reference constructor
 * (Ambiguity.cpp:22-65) and is what its getters return; the second block is
 * this engine's execution plan for the range stage. */
typedef struct blah2hip_amb_dims {
  uint32_t n_doppler_bins; /* Ambiguity::get_n_doppler_bins */
  uint32_t n_delay_bins;   /* Ambiguity::get_n_delay_bins   */
  uint32_t n_corr;         /* Ambiguity::get_n_corr         */
  uint32_t nfft;           /* Ambiguity::get_nfft (value the reference would plan; reported, not used) */
  uint32_t n_samples;      /* constructor argument n        */
  uint32_t n_used;         /* n_corr * n_doppler_bins = samples process() consumes */
  double cpi;              /* Ambiguity::get_cpi            */
  double doppler_middle;   /* Ambiguity::get_doppler_middle */
  uint32_t fft_len;        /* F: on-chip transform length of the range kernel */
  uint32_t n_seg;          /* segments per pulse */
  uint32_t seg_len;        /* reference samples per segment */
  uint32_t max_batch;      /* CPIs one dev call may carry */
} blah2hip_amb_dims_t;

/* One CFAR hit as the device writes it; the host API converts to the
 * reference's Detection triplets. */
typedef struct blah2hip_hit {
  int32_t row; /* Doppler bin index */
  int32_t col; /* delay bin index   */
  double snr;  /* 10*log10|z| - noisePower (CfarDetector1D.cpp:48) */
} blah2hip_hit_t;

/* One final detection as blah2hip_detect_dev writes it: the hit it came from and
 * Detection's triplet after Centroid and Interpolate. */
typedef struct blah2hip_det {
  int32_t row;    /* Doppler bin index of the hit */
  int32_t col;    /* delay bin index of the hit   */
  double delay;   /* bins (Interpolate.cpp:61)    */
  double doppler; /* Hz   (Interpolate.cpp:81)    */
  double snr;     /* dB   (Interpolate.cpp:86)    */
} blah2hip_det_t;

const char *blah2hip_last_error(void);
const char *blah2hip_version(void);
int blah2hip_device_count(int *count);
/* smallest 5-smooth integer strictly greater than v (HammingNumber.cpp:38-48) */
uint32_t blah2hip_next_hamming(uint32_t v);

/* ---- Ambiguity (Ambiguity.h:34-58) ------------------------------------- */
int blah2hip_amb_create(int32_t delay_min, int32_t delay_max, int32_t doppler_min,
                        int32_t doppler_max, uint32_t fs, uint32_t n, int round_hamming,
                        int device, uint32_t max_batch, blah2hip_amb_t *out);
/* Extension (not in the reference, whose constructor only yields odd counts): the same
 * engine with an EXPLICIT number of Doppler bins / pulses, n_doppler_bins (0 = the
 * reference's rule).  nCorr = n / n_doppler_bins, cpi, both axes and the row shift
 * (j + nD/2 + 1) % nD of Ambiguity.cpp:165 follow from it unchanged; for an even count
 * the Nyquist bin is the last row.  This is how "512 / 1024 / 2048 Doppler bins" of
 * BASELINE.json can be had literally. */
int blah2hip_amb_create_ex(int32_t delay_min, int32_t delay_max, int32_t doppler_min, int32_t doppler_max,
                           uint32_t fs, uint32_t n, int round_hamming, uint32_t n_doppler_bins,
                           int device, uint32_t max_batch, blah2hip_amb_t *out);
/* Geometry (the reference's own limit is the uint16 narrowing of Ambiguity.h:80-89, reproduced):
 *   - any number of delay bins: a window of more than 4081 lags runs as chunks of 2048 on the 4096-point range
 *     transform, each chunk re-reading the pulses (correct, slower per bin);
 *   - delays beyond nfft - n_corr read, in the reference's nfft-point CIRCULAR correlation (Ambiguity.cpp:132-146), the
 *     opposite-sign lag d -+ nfft: reproduced (every delay maps to one linear lag; runs of consecutive lags are chunks);
 *     |delay| >= nfft, where the reference indexes outside its buffer, is BLAH2HIP_ERR_UNSUPPORTED;
 *   - Doppler lengths above 2049 run on the direct-DFT kernel (correct, slow). */
int blah2hip_amb_destroy(blah2hip_amb_t h);
int blah2hip_amb_get_dims(blah2hip_amb_t h, blah2hip_amb_dims_t *dims);
/* Map::delay (bins, length n_delay_bins) and Map::doppler (Hz, length n_doppler_bins) */
int blah2hip_amb_get_axes(blah2hip_amb_t h, int32_t *delay, double *doppler);

/* Execution plan, per handle.  Options take effect on the next process call. */
#define BLAH2HIP_OPT_DOPPLER_KERNEL 1 /* BLAH2HIP_DOP_*; AUTO picks by launch size */
#define BLAH2HIP_OPT_RANGE_GRID 2     /* workgroups of the range kernel; 0 = the launched kernel's residency */
#define BLAH2HIP_OPT_RANGE_WALK (BLAH2HIP_OPT_MULTI_SURV_RANGE + 1) /* = 12: how the waves of the _WAVE1K range kernel get their pulses: 0 = the engine's choice,
                                       * BLAH2HIP_WALK_STATIC (wave w of workgroup b of G: pulses b*12 + w + k*G*12) or _TICKET (each
                                       * wave takes its next pulse from one of eight counters when it needs one; the same bits).  Other
                                       * range kernels walk statically whatever this says */
#define BLAH2HIP_WALK_STATIC 1
#define BLAH2HIP_WALK_TICKET 2
#define BLAH2HIP_OPT_RANGE_KERNEL 3   /* 0 = by transform length and launch size (4096: E16; 2048: WAVE once a launch has a pulse per wave
                                       * slot of the chip -- 8 x CUs -- else E16, e.g. a single CPI; 1024: WAVE1K from 12 x CUs pulses,
                                       * else E8); BLAH2HIP_RANGE_E16 / _WAVE (F = 2048) / _WAVE2 (F = 4096, measured 5 % slower than
                                       * E16) / _WAVE1K / _E8 (F = 1024) force one */
#define BLAH2HIP_OPT_DOPPLER_GRID 4   /* workgroup cap of the PERSISTENT Doppler tile kernels (TILE8 / TILE16 / TILEW / TILEW2); 0 = their
                                       * residency (one or two workgroups per CU).  A small cap makes every workgroup walk many tiles --
                                       * the steady state of the software-pipelined loops -- on a small fixture (tests) */
#define BLAH2HIP_OPT_FFT_LEN 5        /* range transform length F in {1024, 2048, 4096}; 0 = the planner's choice (cost model).  Re-plans the
                                       * segmentation and re-uploads the root table (blocking); BLAH2HIP_ERR_UNSUPPORTED when the lag window
                                       * does not fit F.  Replaces the BLAH2HIP_FFT_LEN environment variable of earlier versions */
#define BLAH2HIP_OPT_CFAR2D_KERNEL 6  /* 2-D detector: BLAH2HIP_CFAR2D_AUTO (the one-pass stream kernel for the window shapes it is instantiated
                                       * for -- C2S_SHAPES in csrc/cfar_kernels.hpp, among them config.yml's 2 / 6 along delay with 1 / 3 along
                                       * Doppler --, the one-pass tile kernel for other windows with nGf + nTf <= 24 and nGd + nTd <= 40, else the
                                       * summed-area table), _STREAM / _TILE (BLAH2HIP_ERR_UNSUPPORTED at the call for other windows) or _SAT */
#define BLAH2HIP_OPT_LEAK_COMPENSATION 7 /* Fixed-pattern leak of the fp32 transform chain (csrc/capi.hip, "leak compensation"): the butterfly
                                       * and twiddle constants are each off by up to 3e-8 of themselves, the same way in every transform, and
                                       * what that adds up to over a CPI is a FIXED fraction g[d] (<= 2e-8) of the lag-0 column appearing at a
                                       * few dozen lags d -- in the zero-Doppler row, where the direct-path peak stands sqrt(N) above the floor,
                                       * up to 1e-4 of a floor cell at 4e7 samples per CPI.  g is measured once per (range kernel, Doppler
                                       * kernel) on a synthetic white CPI against its exact fp64 direct sum and subtracted from that row.
                                       * 1 (default): where max|g| sqrt(N) >= 3e-5 (not at 2 MS/s x 1 s); 2: wherever a pattern was measured;
                                       * 0: never.  No reference counterpart (the reference computes in fp64). */
#define BLAH2HIP_OPT_HOT_COLUMNS 8    /* fp64 Doppler transform of the delay columns that hold a peak more than 250x (24 dB) above the map's
                                       * mean level (csrc/capi.hip, "hot columns"): the fp32 transform leaves up to 1.2e-7 of a column's peak
                                       * in that column's other rows, which behind the clutter filter (the floor 8x down, a target 1400x above
                                       * it at 10 MS/s) is 1.7e-4 of a mean-level cell.  At most 16 columns a CPI
                                       * (BLAH2HIP_INFO_HOT_COLUMNS_MISSED counts the rest), found from the range map: the
                                       * larger of two sample standard deviations of the column, over S contiguous pulses and
                                       * over S evenly spaced ones (S = 32 up to nD = 1025, else 48), reads at least 0.8 of a
                                       * tone's amplitude at every Doppler (nD <= 4096), and the test is lowered by that factor.
                                       * 1 (default): CPIs of >= 35 000 samples (a shorter one cannot hold such a peak);
                                       * 2: every call; 0: never.  No reference counterpart (the reference computes in fp64). */
#define BLAH2HIP_OPT_CFAR2D_SEG_ROWS 9 /* Doppler rows per segment of the 2-D stream kernel (a wave walks one segment of one strip of columns);
                                       * 0 = the launch's cost model (8 ... 1024 rows, or the whole map); larger values are clipped to the
                                       * map.  For tests: the seams between segments fall on other rows than a small fixture would give them */
#define BLAH2HIP_OPT_CFAR2D_GRID 10   /* workgroup cap of the PERSISTENT 2-D tile kernel, rounded up to a multiple of 8; 0 = one per CU (or
                                       * per tile).  A small cap makes every workgroup walk many tiles on a small fixture (tests) */
#define BLAH2HIP_OPT_MULTI_SURV_RANGE 11 /* range path of blah2hip_amb_process_multi_dev: BLAH2HIP_MULTI_AUTO (the shared-reference kernel
                                       * where BLAH2HIP_RANGE_WAVE1K would have run and only for the (format, channel count) cases it
                                       * measured faster in), _SHARED (BLAH2HIP_ERR_UNSUPPORTED at the call where
                                       * the kernel does not cover it: F != 1024, asymmetric Doppler limits, a format other than
                                       * FMT_C32 / FMT_I8, another range kernel forced; a lone channel has nothing to share and runs
                                       * the per-channel path) or _PER_CHANNEL (the two-channel range stage once per channel) */
#define BLAH2HIP_OPT_CFAR_LOOKS (BLAH2HIP_OPT_RANGE_WALK + 1) /* = 13: looks per cell L the detectors' threshold factors are made for (blah2hip_cfar_alpha), 1 (default) ..
                                       * BLAH2HIP_MAX_CFAR_LOOKS: L = n_surv * window for the maps of blah2hip_nci_process_dev.  Read by
                                       * blah2hip_cfar1d_dev / _cfar2d_dev / *_process and by *_prepare at the time of the call: the table is
                                       * cached per (pfa, looks, size).  1 builds the table, and gives the bits, of a handle that never saw the
                                       * option.  blah2hip_cfar1d_map takes no handle and stays one-look */
#define BLAH2HIP_MAX_CFAR_LOOKS 1024
#define BLAH2HIP_OPT_TAPER_SEG_ROWS (BLAH2HIP_OPT_CFAR_LOOKS + 1) /* = 14: Doppler rows per segment of taper_kernel (blah2hip_amb_taper_dev: a workgroup walks one segment of one
                                       * strip of 256 columns); 0 = the launch's own choice (32 rows); larger values are clipped to the map,
                                       * smaller ones raised until a map's workgroups fit the handle's metrics partials.  For tests: seams
                                       * and the wrap from row n_doppler - 1 to row 0 fall where a small fixture would not put them */
#define BLAH2HIP_MULTI_AUTO 0
#define BLAH2HIP_MULTI_SHARED 1
#define BLAH2HIP_MULTI_PER_CHANNEL 2
#define BLAH2HIP_CFAR2D_AUTO 0
#define BLAH2HIP_CFAR2D_TILE 1
#define BLAH2HIP_CFAR2D_SAT 2
#define BLAH2HIP_CFAR2D_STREAM 3
#define BLAH2HIP_DOP_AUTO 0
#define BLAH2HIP_DOP_TILE8 1   /* nD <= 513: 8-column tiles, one wave per column */
#define BLAH2HIP_DOP_TILE16 2  /* nD <= 513: 16-column tiles, one wave per column on the one-wave 1024-point transform */
#define BLAH2HIP_DOP_TILEM 3   /* 513 < nD <= 2049: multi-wave columns, 8 or 4 per workgroup */
#define BLAH2HIP_DOP_COLUMN 4  /* nD <= 2049: one column per workgroup (small launches) */
#define BLAH2HIP_DOP_DIRECT 5  /* any nD: direct DFT */
#define BLAH2HIP_DOP_TILEW 6   /* 513 < nD <= 1025: one-wave 2048-point columns, 8 per workgroup */
#define BLAH2HIP_DOP_TILEW2 7  /* 1025 < nD <= 2049: two-wave 4096-point columns, 4 per workgroup */
#define BLAH2HIP_DOP_TILE16WG 8 /* TILE16 on the workgroup transform of rounds 1-2 (twiddles in registers; kept for comparison) */
#define BLAH2HIP_DOP_TILEW4 11 /* 1025 < nD <= 2049: ONE wave per column, the 4096-point transform as four one-wave 1024-point transforms + a radix-4 step in registers, 8 columns per workgroup (round 5) */
#define BLAH2HIP_DOP_TILE8K 10 /* nD <= 513: TILE16's kernel on 8-column half tiles, two workgroups per CU (round 5) */
#define BLAH2HIP_DOP_SUB4 9    /* nD <= 513, small launches (a lone CPI): 4-column workgroups, one wave per SIMD; Map::set_metrics finished by the last workgroup */
#define BLAH2HIP_DOP_PFA513 12 /* nD = 513 only: 16-column tiles, two columns per wave on the 27 x 19 prime-factor transform (no chirp-z); what AUTO runs where it ran TILE16 */
#define BLAH2HIP_RANGE_E16 1   /* 16 points per thread, one workgroup per pulse (F = 4096; F = 2048 on request) */
#define BLAH2HIP_RANGE_E8 2    /* 8 points per thread, last stage across lanes (F = 1024) */
#define BLAH2HIP_RANGE_WAVE 3  /* one wave per pulse, 32 points per lane, no barriers (F = 2048) */
/* 4: was BLAH2HIP_RANGE_WAVE2 (a pair of waves per pulse at F = 4096; measured 5 % slower than _E16 and removed in round 4) */
#define BLAH2HIP_RANGE_WAVE1K 5 /* one wave per pulse, 16 points per lane, four waves per SIMD (F = 1024) */
#define BLAH2HIP_RANGE_FIR 7      /* INFO_LAST_RANGE_KERNEL only: range_fir_kernel (blah2hip_amb_set_fir) */
#define BLAH2HIP_RANGE_PS 6     /* small launches (a lone CPI) at F = 1024: one workgroup of four waves per pulse, its segments dealt round-robin to the waves */
#define BLAH2HIP_RANGE_SHARED 8  /* INFO_LAST_RANGE_KERNEL only: rangew1k_shared_kernel, _WAVE1K for pairs of surveillance channels against
                                  * one reference channel whose transform they share (blah2hip_amb_process_multi_dev, F = 1024) */
/* BLAH2HIP_ERR_UNSUPPORTED when the kernel does not cover the handle's Doppler length */
int blah2hip_amb_set_option(blah2hip_amb_t h, int option, int64_t value);
#define BLAH2HIP_INFO_LAST_DOPPLER_KERNEL 1 /* BLAH2HIP_DOP_* the last process call launched (0 = none yet) */
#define BLAH2HIP_INFO_LAST_RANGE_KERNEL 2   /* BLAH2HIP_RANGE_* */
#define BLAH2HIP_INFO_DOPPLER_FFT_LEN 3     /* chirp-z transform length M (0 = direct DFT only) */
#define BLAH2HIP_INFO_RANGE_GRID 4
#define BLAH2HIP_INFO_NUM_CU 5
#define BLAH2HIP_INFO_DOPPLER_GRID 6        /* workgroups of the last Doppler launch */
#define BLAH2HIP_INFO_LEAK_LAGS 8            /* cells of the zero-Doppler row the last process call corrected (0 = compensation not applied) */
#define BLAH2HIP_INFO_LEAK_MAX_E12 9         /* 1e12 x the largest |g| measured for the kernel pair the last call ran (0 = not measurable: no
                                              * zero-Doppler row / lag-0 column, rotated reference channel, chunked lag window) */
#define BLAH2HIP_INFO_HOT_COLUMNS 10          /* columns of the last call's first CPI rewritten in fp64 (BLAH2HIP_OPT_HOT_COLUMNS); waits for that call's stream */
#define BLAH2HIP_INFO_HOT_COLUMNS_MISSED 11   /* the most columns of any CPI of the last call that passed the hot-column test and were NOT
                                               * rewritten -- beyond the 16 a CPI, or beyond 64 candidates in one quarter of the lags:
                                               * they keep the fp32 floor; waits for that call's stream */
#define BLAH2HIP_INFO_CFAR2D_SEG_ROWS 12     /* rows per segment of the last 2-D detector launch if it was the stream kernel, else 0 */
#define BLAH2HIP_INFO_CFAR2D_GRID 13         /* workgroups of the last 2-D detector launch if it was the tile kernel, else 0 */
#define BLAH2HIP_INFO_DOPPLER_TILES 7       /* tiles (units of work the persistent workgroups walk) of the last Doppler launch; 0 for the
                                             * non-persistent kernels */
#define BLAH2HIP_INFO_DETECT_GRID 14         /* workgroups per CPI of the last blah2hip_detect_dev launch */
#define BLAH2HIP_INFO_DETECT_TILED 15        /* 1: that launch spread a CPI's hits over several workgroups (cap beyond one LDS tile of 1024
                                              * hits), 0: one workgroup per CPI */
#define BLAH2HIP_INFO_BEARING_GRID 16         /* workgroups per list of the last blah2hip_amb_bearing_dev launch */
#define BLAH2HIP_INFO_TAPER_GRID 17            /* workgroups per map of the last blah2hip_amb_taper_dev launch */
#define BLAH2HIP_INFO_MIGRATE_GRID 18          /* workgroups per map of the last blah2hip_amb_migrate_dev launch */
#define BLAH2HIP_INFO_RATE_GRID 19             /* workgroups per map of the last blah2hip_amb_rate_bank_dev launch */
#define BLAH2HIP_INFO_TRACK_GRID 20            /* workgroups per output map of the last track_sum_kernel launch (blah2hip_nci_process_tracks_dev) */
#define BLAH2HIP_INFO_TRACK_MAX_SHIFT 21       /* the largest |s(j,k,a)| of the table the last blah2hip_nci_set_tracks on this handle's maps built */
#define BLAH2HIP_INFO_CARRIER_GRID 22          /* workgroups per map of the last blah2hip_amb_fuse_carriers_dev launch */
int blah2hip_amb_get_info(blah2hip_amb_t h, int key, int64_t *value);

/* Ambiguity::process + Map::set_metrics on host buffers (blah2.cpp:278-279).
 * x = reference, y = surveillance, n complex samples each (n >= n_used, only
 * the first n_used are consumed, like the reference's pops).  map_out may be
 * NULL; metrics[0] = noisePower, metrics[1] = maxPower. */
int blah2hip_amb_process_c64(blah2hip_amb_t h, const double *x, const double *y, uint32_t n,
                             float *map_out, double *metrics);
int blah2hip_amb_process_c32(blah2hip_amb_t h, const float *x, const float *y, uint32_t n,
                             float *map_out, double *metrics);
int blah2hip_amb_process_i16(blah2hip_amb_t h, const int16_t *iq, uint32_t n, float *map_out,
                             double *metrics);
/* x, y: host planes of n int8 (I, Q) pairs each (BLAH2HIP_FMT_I8), uploaded as they are: one CPI */
int blah2hip_amb_process_i8(blah2hip_amb_t h, const int8_t *x, const int8_t *y, uint32_t n, float *map_out,
                            double *metrics);

/* Device-resident chain: range kernel -> Doppler kernel (+ fused metrics).
 * d_x/d_y: device pointers (fmt C32, F16, I8: two planes; fmt I16: d_x = interleaved
 * buffer, d_y ignored; fmt I16X_C32Y, I8X_C32Y: d_x as for I16 / I8, d_y an fp32 plane).
 * CPI c starts at sample c*cpi_stride.  d_map:
 * [n_cpi][n_doppler][n_delay] complex fp32; d_metrics: [n_cpi][2] doubles.
 * Either output may be NULL (then the handle's internal buffer is used and
 * can be read with blah2hip_amb_read_last). */
int blah2hip_amb_process_dev(blah2hip_amb_t h, int fmt, const void *d_x, const void *d_y,
                             uint32_t n_cpi, uint64_t cpi_stride, void *d_map, double *d_metrics,
                             void *stream);
/* One reference channel against n_surv surveillance channels on the same clock (a KrakenSDR: one reference antenna, up to four
 * surveillance antennas).  d_y: HOST array of n_surv device planes, read at the call; every plane has the layout and cpi_stride
 * d_y has above for the same fmt.  fmt: the formats whose surveillance channel is a plane of its own -- FMT_C32, FMT_F16, FMT_I8,
 * FMT_I16X_C32Y, FMT_I8X_C32Y (the two mixed ones are what a clutter filter per channel leaves behind); FMT_I16 is
 * BLAH2HIP_ERR_UNSUPPORTED.  Output, channel-major: d_map [n_surv][n_cpi][n_doppler][n_delay], d_metrics [n_surv][n_cpi][2]
 * (NULL: the handle's buffers, same order).  Channel k of CPI c is thus VIRTUAL CPI k * n_cpi + c for blah2hip_amb_read_last,
 * blah2hip_cfar1d_dev, blah2hip_cfar2d_dev, blah2hip_detect_dev, blah2hip_amb_db_dev and BLAH2HIP_INFO_HOT_COLUMNS*, which are called
 * with n_cpi * n_surv CPIs.  The reference channel is read and transformed once per pair of channels where the shared-reference
 * range kernel runs (BLAH2HIP_OPT_MULTI_SURV_RANGE); everything behind the range map is one launch sequence over the virtual CPIs.
 * n_surv = 1 is blah2hip_amb_process_dev bit for bit.  BLAH2HIP_ERR_INVALID: n_surv == 0 or > BLAH2HIP_MAX_SURV, a NULL plane,
 * n_surv * n_cpi > max_batch; BLAH2HIP_ERR_UNSUPPORTED: a fused FIR set on the handle (blah2hip_amb_set_fir) -- several channels
 * run the two-stage filter per channel. */
#define BLAH2HIP_MAX_SURV 8
int blah2hip_amb_process_multi_dev(blah2hip_amb_t h, int fmt, const void *d_x, const void *const *d_y, uint32_t n_surv,
                                   uint32_t n_cpi, uint64_t cpi_stride, void *d_map, double *d_metrics, void *stream);
/* host planes of n complex fp32 samples each, uploaded, one CPI; map_out [n_surv][n_doppler][n_delay] (may be NULL),
 * metrics [n_surv][2] */
int blah2hip_amb_process_multi_c32(blah2hip_amb_t h, const float *x, const float *const *y, uint32_t n_surv, uint32_t n,
                                   float *map_out, double *metrics);
/* copies CPI `cpi` of the handle's internal map/metrics to the host (synchronises) */
int blah2hip_amb_read_last(blah2hip_amb_t h, uint32_t cpi, float *map_out, double *metrics);
/* The values Map::to_json prints (Map.cpp:148-155): d_db[cpi][doppler][delay] =
 * 10*log10|M| - noisePower as fp32, from d_map/d_metrics as written by
 * blah2hip_amb_process_dev (NULL = the handle's internal buffers).  Enqueues only. */
int blah2hip_amb_db_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi,
                        float *d_db, void *stream);

/* ---- the surveillance channels as ONE array (no reference counterpart) -----
 * Beams in the map domain.  The cross-ambiguity map is linear in the surveillance channel: the beam
 * y_b = sum_k w[b][k] y_k has the map M_b = sum_k w[b][k] M_k, so every beam costs one pass over the K maps that
 * blah2hip_amb_process_multi_dev left in HBM, not a range + Doppler chain.
 * d_map: [n_surv][n_cpi][n_doppler][n_delay] complex fp32 as that call writes it (NULL = the handle's internal map).
 * w: HOST array [n_beams][n_surv] of (re, im) fp32 pairs, read at the call and carried in the launch arguments: no upload,
 * no allocation, no synchronisation; the call enqueues only and can be captured in a graph.
 * Output, beam-major: d_beam_map [n_beams][n_cpi][n_doppler][n_delay], d_beam_metrics [n_beams][n_cpi][2] (Map::set_metrics of
 * every beam map, on the cells as written).  Beam b of CPI c is thus VIRTUAL CPI b * n_cpi + c for blah2hip_cfar1d_dev,
 * blah2hip_cfar2d_dev, blah2hip_detect_dev and blah2hip_amb_db_dev, which are called with n_beams * n_cpi CPIs and these two
 * buffers.  Under noise a beam map is a complex Gaussian field like a channel map, so the detectors' pfa holds per beam map.
 * Every cell is accumulated in fp32 in the order k = 0 .. n_surv - 1; a weight of exactly 1 or 0 passes cells through bit for
 * bit.  One kernel reads the K maps once and writes the n_beams maps once, (n_surv + n_beams) * cells * 8 bytes per CPI; the
 * metrics are finished by metrics_kernel in index order (no floating-point atomics: two calls give the same bits).  The
 * per-workgroup partials live in the handle's buffers, so calls on one handle must be ordered on the device.
 * BLAH2HIP_ERR_INVALID, with nothing enqueued: n_surv outside [1, BLAH2HIP_MAX_SURV], n_beams outside
 * [1, BLAH2HIP_MAX_BEAMS], n_cpi == 0, n_surv * n_cpi or n_beams * n_cpi above max_batch, a NULL w or output, an output
 * that overlaps the input maps (the handle's internal map when d_map is NULL). */
#define BLAH2HIP_MAX_BEAMS 8
int blah2hip_amb_beamform_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_surv, uint32_t n_cpi,
                              const float *w, uint32_t n_beams,
                              void *d_beam_map, double *d_beam_metrics, void *stream);
/* The same beams with weights that differ from CPI to CPI and live on the device: d_w is a DEVICE array
 * [n_cpi][n_beams][n_surv] of (re, im) fp32 pairs, as blah2hip_amb_mvdr_weights_dev writes it; beam b of CPI c is
 * M_b(c) = sum_k d_w[c][b][k] M_k(c).  Everything else is blah2hip_amb_beamform_dev: outputs, virtual-CPI order, metrics,
 * alignment handling, error cases (a NULL d_w for a NULL w) and the BLAH2HIP_K_BEAM / _METRICS slots.  The kernel is a second
 * instantiation of beamform_kernel that reads its CPI's weights once before the first cell; per cell the operations and
 * their order are the same, so weights equal to a beamform_dev call's give that call's bits, maps and metrics.  d_w is read
 * when the kernel runs: whatever writes it must be ordered before this call on the device.  Enqueues only. */
int blah2hip_amb_beamform_wdev(blah2hip_amb_t h, const void *d_map, uint32_t n_surv, uint32_t n_cpi,
                               const float *d_w, uint32_t n_beams,
                               void *d_beam_map, double *d_beam_metrics, void *stream);
/* ---- adaptive beams: array covariance -> minimum-variance (MVDR / Capon) weights -> blah2hip_amb_beamform_wdev ----
 * The array covariance of the channel maps over a training rectangle of cells, per CPI:
 *   d_cov[c][i][j] = sum over row0 <= r < row1, col0 <= q < col1 of M_i(c; r, q) conj(M_j(c; r, q))
 * as (re, im) doubles, shape [n_cpi][n_surv][n_surv]; the whole map is 0, n_doppler, 0, n_delay.  d_map as for
 * blah2hip_amb_beamform_dev (NULL = the handle's internal map).  Both triangles are written, d_cov[c][j][i] is the exact
 * conjugate of d_cov[c][i][j] and the diagonal's imaginary part is exactly 0.
 * Arithmetic: the product of two fp32 values is exact in fp64, and every accumulation -- in the thread, the workgroup and
 * the final fold -- is fp64 (fused multiply-adds in the thread), so the error is that of an fp64 sum of n terms; the
 * contract callers may rely on is the weaker |error| <= 4 * 2^-24 * sum |M_i| |M_j| (fp32 products allowed).  No
 * floating-point atomics: array_cov_kernel leaves one partial per workgroup and cov_fold_kernel adds them in index order, so
 * two calls give the same bits.  The partials live in the handle's metrics partials (max_batch * nParts doubles; the
 * workgroups per CPI are bounded so that n_cpi * G * n_surv^2 fits), which blah2hip_amb_beamform_dev and the process calls use
 * too: calls on one handle must be ordered on the device.  No allocation, upload or synchronisation: the call enqueues only
 * (two kernels, both under BLAH2HIP_K_COV) and can be captured in a graph.
 * BLAH2HIP_ERR_INVALID, with nothing enqueued: NULL handle or output, n_surv outside [1, BLAH2HIP_MAX_SURV], n_cpi == 0,
 * n_surv * n_cpi above max_batch, an empty or out-of-range rectangle (row0 >= row1, row1 > n_doppler, col0 >= col1,
 * col1 > n_delay), d_cov overlapping the input maps. */
int blah2hip_amb_covariance_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_surv, uint32_t n_cpi,
                                uint32_t row0, uint32_t row1, uint32_t col0, uint32_t col1,
                                double *d_cov, void *stream);
/* Minimum-variance distortionless-response weights per CPI c and beam b from d_cov [n_cpi][n_surv][n_surv] (as above; the
 * lower triangle is read) and the steering vectors a_b -- steer: HOST array [n_beams][n_surv] of (re, im) fp32 pairs, read at
 * the call and carried in the launch arguments like w of blah2hip_amb_beamform_dev:
 *   R_l = R[c] + loading * (tr R[c] / n_surv) * I,   h_b = R_l^-1 a_b / (a_b^H R_l^-1 a_b),   d_w[c][b][k] = conj(h_b[k])
 * complex fp32, shape [n_cpi][n_beams][n_surv]: the d_w of blah2hip_amb_beamform_wdev (M_b = sum_k w[b][k] M_k).  The beam is
 * distortionless, sum_k d_w[c][b][k] a_b[k] = 1, and R = I gives conj(a_b) / n_surv for unit-modulus a_b.  The solve is an
 * fp64 Cholesky factorisation with forward and back substitution (mvdr_weights_kernel, one workgroup per CPI, one thread per
 * beam); only the result is rounded to fp32.
 * d_ok[c] (int32, may be NULL): 1 where the factorisation succeeded, 0 where a pivot was not finite or not positive (an
 * all-zero CPI, a NaN in the maps); a failed CPI's weights are the conventional conj(a_b) / (a_b^H a_b), so whatever follows
 * still runs, and the other CPIs of the batch are unaffected.  Enqueues ONE kernel; no allocation or synchronisation.
 * BLAH2HIP_ERR_INVALID, with nothing enqueued: a NULL handle, d_cov, steer or d_w, n_surv outside [1, BLAH2HIP_MAX_SURV],
 * n_beams outside [1, BLAH2HIP_MAX_BEAMS], n_cpi == 0, loading negative or not finite, a steering vector that is all zero. */
int blah2hip_amb_mvdr_weights_dev(blah2hip_amb_t h, const double *d_cov, uint32_t n_surv, uint32_t n_cpi,
                                  const float *steer, uint32_t n_beams, double loading,
                                  float *d_w, int32_t *d_ok, void *stream);
/* ---- the array in the SAMPLE domain: covariance and beam planes in front of the whole chain ----
 * The beam y_b[n] = sum_k w[b][k] y_k[n] is linear in the channels like the clutter filter and the map, so a beam plane formed
 * from the samples is an ordinary surveillance channel: ONE clutter filter, range pass and Doppler pass per beam instead of one
 * per channel, and a covariance estimated where the direct path and the clutter dominate (a target lies far under the noise
 * per sample, so nothing has to be kept out of the training window).
 * d_y: HOST array of n_surv device planes as in blah2hip_amb_process_multi_dev, CPI c at c * cpi_stride samples, the handle's
 * n_samples samples per CPI.  fmt: BLAH2HIP_FMT_C32 (planes of complex fp32, 8-byte aligned) or BLAH2HIP_FMT_I8 (planes of int8
 * (I, Q) pairs, 2-byte aligned); any other format: BLAH2HIP_ERR_UNSUPPORTED.
 *
 * The sample covariance over the window [s0, s1) of every CPI (0, n_samples: all of it):
 *   d_cov[c][i][j] = sum over s0 <= n < s1 of y_i[c * cpi_stride + n] conj(y_j[c * cpi_stride + n])
 * in the layout and with the properties of blah2hip_amb_covariance_dev's output -- (re, im) doubles [n_cpi][n_surv][n_surv], both
 * triangles, exact conjugates, the diagonal's imaginary part exactly 0 -- so it feeds blah2hip_amb_mvdr_weights_dev and
 * blah2hip_amb_bearing_dev unchanged.  Arithmetic, FMT_C32: that call's (fp64 fused multiply-adds on the exactly converted
 * values, every addition fp64); the contract is |error| <= 4 * 2^-24 * sum |y_i| |y_j| per entry.  FMT_I8: the result is
 * EXACT -- every product and every partial sum is an integer below 2^53 -- and so the same whatever the grid.  No
 * floating-point atomics; sample_cov_kernel leaves one partial per workgroup in the handle's metrics partials (the workgroups
 * per CPI are bounded as for blah2hip_amb_covariance_dev; calls on one handle must be ordered on the device) and
 * cov_fold_kernel adds them in index order: two calls give the same bits.  Accesses of several samples (16 bytes of fp32 pairs,
 * 8 bytes of int8 pairs) are used where, CPI by CPI, every plane's window starts at the same offset modulo the access;
 * any other bases and strides go one sample per access.  Enqueues only (two kernels, both under BLAH2HIP_K_COV): no
 * allocation, upload or synchronisation, capturable in a graph.
 * BLAH2HIP_ERR_INVALID, with nothing enqueued: a NULL handle, plane array, plane or output, n_surv outside
 * [1, BLAH2HIP_MAX_SURV], n_cpi == 0, n_surv * n_cpi above max_batch, s0 >= s1 or s1 > n_samples, cpi_stride < n_samples with
 * n_cpi > 1, an int8 plane at an odd address (an fp32 plane off 8 bytes), d_cov overlapping an input plane. */
int blah2hip_amb_sample_covariance_dev(blah2hip_amb_t h, int fmt, const void *const *d_y, uint32_t n_surv,
                                       uint32_t n_cpi, uint64_t cpi_stride, uint32_t s0, uint32_t s1,
                                       double *d_cov, void *stream);
/* Beam planes: d_beam[b][c * beam_stride + n] = sum_k w[b][k] y_k[c * cpi_stride + n], n < n_samples, complex fp32.  w: HOST
 * array [n_beams][n_surv] of (re, im) fp32 pairs, read at the call and carried in the launch arguments, as in
 * blah2hip_amb_beamform_dev.  d_beam: HOST array of n_beams device planes (8-byte aligned).  Samples n >= n_samples of an output
 * CPI -- the gap up to beam_stride -- are not written.  Each beam plane is a valid d_y for blah2hip_clutter_process_dev_fmt
 * (FMT_C32), for blah2hip_amb_process_dev with FMT_C32, FMT_I8X_C32Y or FMT_I16X_C32Y and for blah2hip_amb_process_multi_dev.
 * One kernel (beam_samples_kernel, BLAH2HIP_K_BEAM) reads the n_surv planes once and writes the n_beams planes once.  Per
 * sample and beam the sum is the fp32 fused-multiply-add chain of blah2hip_amb_beamform_dev in the order k = 0 .. n_surv - 1:
 * |error| <= 4 (n_surv + 1) * 2^-24 * sum_k |w_k| |y_k|; a weight of exactly 1 or 0 passes an fp32 sample through bit for bit and
 * an int8 sample as its exact conversion.  16-byte stores (pairs of samples) where, CPI by CPI, every input and every beam
 * plane starts at the same parity of sample; single samples otherwise.  Enqueues only: no allocation, upload or
 * synchronisation, capturable in a graph.
 * BLAH2HIP_ERR_INVALID, with nothing enqueued: a NULL handle, plane array, plane, w or output, n_surv outside
 * [1, BLAH2HIP_MAX_SURV], n_beams outside [1, BLAH2HIP_MAX_BEAMS], n_cpi == 0, cpi_stride or beam_stride < n_samples with
 * n_cpi > 1, an int8 plane at an odd address (an fp32 plane, in or out, off 8 bytes), a beam plane that overlaps an input plane
 * or another beam plane. */
int blah2hip_amb_beam_samples_dev(blah2hip_amb_t h, int fmt, const void *const *d_y, uint32_t n_surv,
                                  uint32_t n_cpi, uint64_t cpi_stride, const float *w, uint32_t n_beams,
                                  void *const *d_beam, uint64_t beam_stride, void *stream);
/* The same with weights that differ from CPI to CPI and live on the device: d_w is a DEVICE array [n_cpi][n_beams][n_surv] of
 * (re, im) fp32 pairs, as blah2hip_amb_mvdr_weights_dev writes it.  beam_samples_wdev_kernel reads its CPI's weights once
 * before the first sample; per sample the operations and their order are the same, so weights equal to a
 * blah2hip_amb_beam_samples_dev call's give that call's bits.  d_w is read when the kernel runs: whatever writes it must be
 * ordered before this call on the device.  Everything else, error cases included (a NULL d_w for a NULL w), as above. */
int blah2hip_amb_beam_samples_wdev(blah2hip_amb_t h, int fmt, const void *const *d_y, uint32_t n_surv,
                                   uint32_t n_cpi, uint64_t cpi_stride, const float *d_w, uint32_t n_beams,
                                   void *const *d_beam, uint64_t beam_stride, void *stream);
/* The array snapshot under every detection: d_snap[l][i][k] = cell (row_i, col_i) of CHANNEL map k of CPI l mod n_cpi, complex
 * fp32, shape [n_lists][cap][n_surv] (re, im) -- what phase differences, a Bartlett or MUSIC bearing or a monopulse ratio are
 * computed from without downloading K maps.  d_dets [n_lists][cap] and d_count [n_lists] as blah2hip_detect_dev leaves them
 * (a count beyond cap: cap records).  List l belongs to CPI l mod n_cpi: the lists of n_beams * n_cpi beam maps and of
 * n_surv * n_cpi channel maps (virtual CPIs) both fit.  d_map as above (NULL = the handle's internal map).  Slots beyond a
 * list's count and records whose row or col lies outside the map are left unwritten.  Enqueues ONE kernel.
 * BLAH2HIP_ERR_INVALID: a NULL list / count / output, cap == 0, n_cpi == 0, n_lists == 0 or not a multiple of n_cpi, n_surv
 * outside [1, BLAH2HIP_MAX_SURV], n_surv * n_cpi above max_batch. */
int blah2hip_amb_snapshot_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_surv, uint32_t n_cpi,
                              const blah2hip_det_t *d_dets, uint32_t cap, const uint32_t *d_count, uint32_t n_lists,
                              float *d_snap, void *stream);
/* The bearing of every detection: the angle scan of its array snapshot s (the n_surv channel cells under the record, gathered
 * from d_map as blah2hip_amb_snapshot_dev gathers them; no snapshot buffer in between) over a steering table a_g,
 * g = 0 .. n_grid - 1 -- d_steer, a DEVICE array [n_grid][n_surv] of (re, im) fp32 pairs: any array geometry, the call knows
 * no angles.  With d_cov [n_cpi][n_surv][n_surv] as blah2hip_amb_covariance_dev writes it (the lower triangle is read) it is
 * the adaptive matched filter's scan, which reads the target's bearing in a cell that also holds an interferer the
 * covariance has seen; with d_cov NULL it is the conventional (Bartlett) scan:
 *   R_l = R[c] + loading * (tr R[c] / n_surv) * I = L L^H   (Cholesky, formed as blah2hip_amb_mvdr_weights_dev forms it;
 *                                                            d_cov NULL: L = I)
 *   v_g = L^-1 a_g,  t = L^-1 s,  P(g) = |v_g^H t|^2 / (v_g^H v_g)   (0 where v_g^H v_g is 0)
 *   index     = argmax P, the LOWEST g on an exact tie
 *   offset    = (P- - P+) / (2 (P- - 2 P0 + P+)) on the linear powers at index - 1, index, index + 1: a fraction of a grid step
 *               to add to index; 0 where the denominator is not negative
 *   power     = P(index),   coherence = P(index) / (t^H t), in [0, 1]: 1 for a noise-free plane wave on the grid
 * Ends of the grid: with BLAH2HIP_BEARING_WRAP the grid is a closed circle (360 degrees of a circular array) and the
 * neighbours of index 0 and n_grid - 1 wrap; without it a peak at an end has offset 0.  A snapshot that is all zero or not
 * finite gives index -1 and zeros in the other fields.  A CPI whose factorisation meets a pivot that is not finite or not
 * positive (an all-zero CPI, a NaN in the maps) falls back to L = I and marks its records adaptive = 0; the other CPIs of
 * the batch are unaffected, bit for bit -- the rule of blah2hip_amb_mvdr_weights_dev.  An identity covariance with loading 0
 * gives the bits of the d_cov = NULL call in every field but adaptive.
 * d_dets [n_lists][cap], d_count [n_lists], the rule that list l belongs to CPI l mod n_cpi (maps and covariance) and d_map are
 * those of blah2hip_amb_snapshot_dev; d_out is [n_lists][cap].  Slots beyond a list's count (a count beyond cap: cap
 * records) and records whose row or col lies outside the map are left unwritten.
 * Arithmetic: everything is fp64 -- the fp32 cells and steering entries convert exactly, the table is whitened and
 * normalised in fp64 (bearing_kernel: once per workgroup into LDS, then one wave per detection, lanes over g) and nothing
 * is rounded to fp32.  No atomics: two calls give the same bits.  Enqueues ONE kernel (BLAH2HIP_K_BEARING); no allocation,
 * upload or synchronisation, and the call can be captured in a graph.  d_cov, d_steer, the lists and the maps are read when
 * the kernel runs: whatever writes them must be ordered before this call on the device.
 * BLAH2HIP_ERR_INVALID, with nothing enqueued: a NULL handle, list, count, steering table or output, cap == 0, n_cpi == 0,
 * n_lists == 0, not a multiple of n_cpi or above 65535, n_surv outside [2, BLAH2HIP_MAX_SURV], n_surv * n_cpi above
 * max_batch, n_grid outside [3, BLAH2HIP_MAX_BEARING_GRID], unknown flag bits, loading negative or not finite when d_cov is
 * not NULL. */
#define BLAH2HIP_MAX_BEARING_GRID 384     /* 360 degrees in 1 degree steps fits */
#define BLAH2HIP_BEARING_WRAP 1u
typedef struct blah2hip_bearing {
  int32_t index;      /* grid index of the peak, -1: no estimate */
  int32_t adaptive;   /* 1: the CPI's covariance was used, 0: Bartlett (d_cov NULL or a failed factorisation) */
  double offset;      /* fraction of a grid step, added to index */
  double power;
  double coherence;
} blah2hip_bearing_t;
int blah2hip_amb_bearing_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_surv, uint32_t n_cpi,
                             const blah2hip_det_t *d_dets, uint32_t cap, const uint32_t *d_count, uint32_t n_lists,
                             const double *d_cov, double loading,
                             const float *d_steer, uint32_t n_grid, uint32_t flags,
                             blah2hip_bearing_t *d_out, void *stream);

/* ---- non-coherent integration over channels and CPIs (no reference counterpart) ----
 * Two ways to more sensitivity than one map gives, in one pass: the sum of |M_k|^2 over the surveillance channels, which
 * unlike the beams above needs no phase calibration of the array, and the sum over a sliding window of W consecutive CPIs.
 * With the maps M_k[g] of CPI g, channel weights w_k >= 0 (receivers of unequal gain; default 1), window W and hop H:
 *   p[g][cell]   = sum_k w_k |M_k[g][cell]|^2                            fp32, k ascending
 *   out[g][cell] = ( sqrtf(scale * (p[g-W+1] + ... + p[g])), 0 )          fp32, oldest CPI first
 *   scale        = 1 / (W * sum_k w_k), rounded to fp32 on the host
 * for every g >= W - 1 with (g - (W - 1)) % H == 0; g counts the CPIs the integrator has seen since its creation or its
 * last reset, across calls (H > W: the CPIs between two windows are not used).  The output is an ordinary complex map --
 * the RMS level in the real part, a zero imaginary part -- so |z|^2 is the normalised sum and 10 log10|z| its level, and
 * blah2hip_cfar1d_dev, blah2hip_cfar2d_dev, blah2hip_detect_dev, blah2hip_amb_db_dev and the JSON writers run on the n_out
 * output maps unchanged, as virtual CPIs 0 .. n_out - 1.  Under noise a cell of the sum is Gamma distributed with
 * L = n_surv * W looks, not exponential: set BLAH2HIP_OPT_CFAR_LOOKS to L for the detectors' pfa to hold
 * (blah2hip_cfar_alpha).  With unequal weights L is only nominal -- the sum is no longer Gamma(L), its effective looks are
 * (sum w)^2 / sum w^2 -- and the caller chooses the value.
 * No running sums: every window is added up on its own, so nothing drifts, and a NaN or Inf cell of CPI g touches the
 * windows that contain g and no other.  The integrator keeps p of the last W - 1 CPIs as fp32 planes, 4 (W - 1) cells bytes,
 * written with the values the call summed: the bits of out[g], and of its metrics, do not depend on how the CPIs were cut
 * into calls.  Per cell a term passes n_surv + 2 roundings on its way into p, at most W - 1 additions, the scale and the
 * square root; all terms are non-negative, so the error is below (n_surv * W + 8) 2^-24 of the cell. */
#define BLAH2HIP_MAX_NCI_WINDOW 16
typedef struct blah2hip_nci_s *blah2hip_nci_t;
/* An integrator for the maps of `amb` (its geometry; n_surv channels per CPI, window W, hop H), counter 0.  Allocates the
 * history planes.  BLAH2HIP_ERR_INVALID: a NULL argument, n_surv outside [1, BLAH2HIP_MAX_SURV], window outside
 * [1, BLAH2HIP_MAX_NCI_WINDOW], hop == 0.  (BLAH2HIP_ERR_UNSUPPORTED: the handle has fewer metrics partials per map than
 * the kernel has workgroups, one per 512 cells; no geometry the engine plans today.) */
int blah2hip_nci_create(blah2hip_amb_t amb, uint32_t n_surv, uint32_t window, uint32_t hop, blah2hip_nci_t *out);
/* Waits for the device (enqueued calls use the history) and frees it.  Call it BEFORE blah2hip_amb_destroy of its handle. */
int blah2hip_nci_destroy(blah2hip_nci_t n);
/* g = 0 and the history forgotten: the next window needs W new CPIs.  Host only, enqueues nothing (calls enqueued
 * earlier are not affected). */
int blah2hip_nci_reset(blah2hip_nci_t n);
/* What blah2hip_nci_process_dev would report for the next n_cpi CPIs, without enqueuing or counting anything: *n_out, the
 * windows that end inside them, and *first_end, the g of the first window that ends at or behind the counter (inside the
 * n_cpi CPIs exactly when *n_out > 0; the later ones follow every H).  Pure functions of the counter, n_cpi, W and H;
 * either pointer may be NULL. */
int blah2hip_nci_count(blah2hip_nci_t n, uint32_t n_cpi, uint32_t *n_out, uint64_t *first_end);
/* The next n_cpi CPIs.  d_map: [n_surv][n_cpi][n_doppler][n_delay] complex fp32 as blah2hip_amb_process_multi_dev writes
 * it (n_surv = 1: a single channel's maps; beam maps work as well; NULL = the handle's internal map).  w: HOST array
 * [n_surv] of fp32 weights, read at the call and carried in the launch arguments, or NULL for all 1.  Output: d_out_map
 * [n_out][n_doppler][n_delay], window after window, and d_out_metrics [n_out][2], Map::set_metrics of every output map on
 * the cells as written.  *n_out and *first_end as blah2hip_nci_count reports them (either may be NULL): they are computed
 * on the host, so the call only enqueues -- no allocation, upload or synchronisation -- and can be captured in a graph
 * (a replay repeats the launch, not the count).  n_out may be 0, while the window fills: nothing is written to the
 * outputs (they may be NULL), the history is still updated.
 * One kernel (nci_kernel, BLAH2HIP_NK_NCI) reads every input cell once, whatever W and H are, reads the history planes at
 * its start and writes them at its end; metrics_kernel finishes the metrics in index order (no floating-point atomics:
 * two calls give the same bits).  The per-workgroup partials live in the ambiguity handle's buffers, so calls on one
 * handle -- this one, the process calls, the beam former -- must be ordered on the device.
 * BLAH2HIP_ERR_INVALID, with nothing enqueued and the counter unchanged: a NULL handle, n_cpi == 0, n_surv * n_cpi above
 * max_batch, n_out above out_cap or above max_batch, a weight that is negative or not finite, weights that add up to 0, a
 * NULL output while n_out > 0, a map that is not 8-byte aligned, an output that overlaps the input maps (the handle's
 * internal map when d_map is NULL), an integrator with tracks set (blah2hip_nci_set_tracks: its history lives in the ring). */
int blah2hip_nci_process_dev(blah2hip_nci_t n, const void *d_map, uint32_t n_cpi, const float *w,
                             void *d_out_map, double *d_out_metrics, uint32_t out_cap,
                             uint32_t *n_out, uint64_t *first_end, void *stream);

/* ---- Doppler taper (no reference counterpart: Ambiguity.cpp:152-169 transforms the pulses unwindowed) ----
 * A cosine-sum slow-time window  w[i] = sum_{p=0..P} (-1)^p a_p cos(2 pi p i / n_doppler),  i = pulse 0 .. n_doppler - 1 (the
 * periodic, "DFT-even" form), multiplied onto the range rows in front of the Doppler transform equals a real, symmetric
 * (2P + 1)-tap CIRCULAR stencil along the Doppler rows of the finished map,
 *   M'[j][d] = t_0 M[j][d] + sum_{m=1..P} t_m ( M[(j-m) mod n_doppler][d] + M[(j+m) mod n_doppler][d] ),
 *   t_0 = a_0,  t_m = (-1)^m a_m / 2
 * (the map's row order is a rotation of the transform's, so circular neighbours stay neighbours and rows 0 and
 * n_doppler - 1 are adjacent -- for odd n_doppler and for the explicit even n_doppler_bins alike).  The taper is therefore
 * one kernel over maps that are already on the device, and composes with everything that takes a d_map / d_metrics pair:
 * the integrator, the detectors, the finisher, the beam former.  Arithmetic, per component, fp32, in this order:
 *   acc = t_0 * M[j];   for m = 1 .. P:  acc = fmaf(t_m, M[j-m], acc);  acc = fmaf(t_m, M[j+m], acc)
 * -- 2P + 1 roundings, each at most 2^-24 of B = sum_m |t_m| |M[j+m]| (m = -P .. P), in one fixed order: equal inputs give
 * equal bits at every placement, segmentation and cut into calls; n_side = 0 with t_0 = 1 copies the cells bit for bit.
 * A NaN cell makes the 2P + 1 cells of its column whose stencil holds it NaN and no other.  Along delay the cells stay
 * independent (the 1-D detectors' pfa holds); along Doppler neighbours within P bins are correlated. */
#define BLAH2HIP_MAX_TAPER_SIDE 4
#define BLAH2HIP_TAPER_NONE 0            /* t_0 = 1, n_side 0 */
#define BLAH2HIP_TAPER_HANN 1            /* a = 0.5, 0.5 */
#define BLAH2HIP_TAPER_HAMMING 2         /* a = 0.54, 0.46 */
#define BLAH2HIP_TAPER_BLACKMAN 3        /* a = 0.42, 0.5, 0.08 */
#define BLAH2HIP_TAPER_BLACKMAN_HARRIS 4 /* a = 0.35875, 0.48829, 0.14128, 0.01168 */
#define BLAH2HIP_TAPER_NUTTALL 5         /* a = 0.3635819, 0.4891775, 0.1365995, 0.0106411 */
#define BLAH2HIP_TAPER_FLATTOP 6         /* a = 0.21557895, 0.41663158, 0.277263158, 0.083578947, 0.006947368 */
/* Host only: the taps t_0 .. t_4 of a named window (those behind n_side are 0) and its half width.  normalise != 0 divides
 * by a_0: an echo on a Doppler bin keeps its amplitude.  taps: BLAH2HIP_MAX_TAPER_SIDE + 1 floats, the fp32 roundings of
 * the fp64 values.  BLAH2HIP_ERR_INVALID: an unknown kind, a NULL argument. */
int blah2hip_doppler_taper(int kind, int normalise, float *taps, uint32_t *n_side);
/* M' = stencil(M) for n_maps maps [n_doppler][n_delay] complex fp32 -- CPIs, virtual CPIs of channels or beams: any maps of
 * this handle's geometry.  d_map NULL = the handle's internal map.  taps: HOST array of n_side + 1 floats, read at the call
 * and carried in the launch arguments (any real taps, not only the named windows').  Outputs: d_out_map [n_maps][n_doppler]
 * [n_delay] and d_out_metrics [n_maps][2], Map::set_metrics of every output map on the cells as written.  Enqueues only --
 * taper_kernel (BLAH2HIP_K_BEAM) and metrics_kernel (BLAH2HIP_K_METRICS), which finishes the metrics in index order (no
 * floating-point atomics) -- with no upload, allocation or synchronisation, and can be captured in a graph.  The grid
 * depends on the map's geometry and BLAH2HIP_OPT_TAPER_SEG_ROWS alone, never on n_maps: a map's cells and metrics are the
 * same bits however the maps are cut into calls.  The per-workgroup partials live in the handle's buffers, so calls on
 * one handle must be ordered on the device.  Maps may sit at any 8-byte aligned address: every access is 8 bytes per lane,
 * 512 contiguous bytes a wave, the same kernel and the same bits at every placement.
 * BLAH2HIP_ERR_INVALID, with nothing enqueued: a NULL handle, n_side above BLAH2HIP_MAX_TAPER_SIDE, n_doppler below
 * 2 n_side + 1, n_maps 0 or above max_batch, NULL taps or outputs, a tap that is not finite, a map that is not 8-byte
 * aligned, an output that overlaps the input maps (the stencil cannot run in place). */
int blah2hip_amb_taper_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_maps, const float *taps, uint32_t n_side,
                           void *d_out_map, double *d_out_metrics, void *stream);

/* ---- Range-migration compensation (no reference counterpart: Ambiguity.cpp:152-169 sums the pulses of one delay column) ----
 * A target's bistatic delay drifts over a CPI by -f n_used / fc samples (f Doppler, fc carrier), so a fast echo leaves its
 * delay column part-way through the Doppler sum and smears over the cells it walks through.  The compensation is a second
 * Doppler sum over the range map of the last process call, which stays on the handle, taken along the walk.  With
 *   R[i][d]   the range map of one (virtual) CPI: pulse i, delay column d = 0 .. n_delay - 1,
 *   src(j)  = (j + n_doppler/2 + 1) % n_doppler   (the map's row order),   W[m] = exp(-2 pi i m / n_doppler),
 *   h[j]      a table of fp64 HALF WALKS: samples per pulse, divided by 2,
 *   t(i)    = 2 i - (n_doppler - 1)                                   (an integer, for odd and even n_doppler alike)
 *   s(j,i)  = (int) rint( h[j] * (double) t(i) )                      (one fp64 multiply, ties to even)
 *   M'[j][d] = sum_i [0 <= d + s(j,i) < n_delay]  R[i][d + s(j,i)] W[(i src(j)) mod n_doppler]
 * A term whose column falls outside the map contributes zero: no wrap, no clamp.  The shift is to the nearest cell (no
 * interpolation).  A ZERO-SHIFT row -- rint(h[j] (n_doppler - 1)) == 0, so every s(j,i) is 0 -- is copied bit for bit from
 * the input map: the rows around zero Doppler keep what the hot-column and leak machinery wrote.  Every other row is
 * overwritten by the sum, in doppler_dft_kernel's arithmetic without its first-pulse subtraction: fp32 complex
 * multiply-adds, blocks of 32 pulses summed into a running sum, in one fixed order, so equal inputs give equal bits at every
 * placement and every n_maps. */
#define BLAH2HIP_MAX_MIGRATION 512 /* the largest |rint(h[j] (n_doppler - 1))| a table may hold: cells walked from the middle of the CPI to its end */
/* Host only: the physical table of the handle's own Doppler axis, half_walk[j] = -0.5 * doppler[j] * n_corr / fc for
 * j = 0 .. n_doppler - 1.  Positive Doppler is an approaching target, whose delay decreases; the echo lands at its mid-CPI
 * delay.  BLAH2HIP_ERR_INVALID: a NULL argument, fc not finite or not positive. */
int blah2hip_migration_table(blah2hip_amb_t h, double fc, double *half_walk);
/* Copies a HOST table of n_doppler half walks into a device buffer the handle owns (allocated at the first call; the call
 * waits for the device, like blah2hip_amb_set_fir's tables).  Any finite table is allowed, not only the physical one.  NULL
 * clears the table.  BLAH2HIP_ERR_INVALID, with the table that was set left as it was: an entry that is not finite, or
 * max_j |rint(h[j] (n_doppler - 1))| above BLAH2HIP_MAX_MIGRATION. */
int blah2hip_amb_set_migration(blah2hip_amb_t h, const double *half_walk);
/* M' for maps 0 .. n_maps - 1 of the handle's range map AS THE LAST blah2hip_amb_process_dev / _process_multi_dev CALL LEFT
 * IT (virtual CPIs k * n_cpi + c).  d_map: that call's map buffer (NULL = the handle's own), read in zero-shift rows only.
 * d_out_map [n_maps][n_doppler][n_delay] may be the same pointer (in place) or a disjoint buffer; d_out_metrics [n_maps][2]
 * is Map::set_metrics of every output map on the cells as written.  Enqueues only -- walk_sum_kernel<8, 1> (BLAH2HIP_K_DOPPLER)
 * and metrics_kernel (BLAH2HIP_K_METRICS), which finishes the metrics in index order (no floating-point atomics) -- with
 * no upload, allocation or synchronisation, and can be captured in a graph.  The grid depends on the geometry alone, never
 * on n_maps.  The per-workgroup partials live in the handle's buffers, so calls on one handle must be ordered on the device.
 * BLAH2HIP_ERR_INVALID, with nothing enqueued: a NULL handle, no table set, no process call yet, n_maps 0 or above the
 * maps of the last process call, NULL outputs, a map that is not 8-byte aligned, output maps that overlap the input maps
 * without being the same pointer, a metrics buffer inside a map. */
int blah2hip_amb_migrate_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_maps, void *d_out_map, double *d_out_metrics,
                             void *stream);

/* ---- Doppler-rate bank (no reference counterpart: Ambiguity.cpp:152-169 sums every pulse with one fixed Doppler) ----
 * A target whose bistatic range accelerates by a m/s^2 drifts in Doppler by -a fc / c Hz per second: over the CPI of
 * T = n_doppler n_corr / fs seconds that is q = -a fc / c T^2 Doppler bins, and the echo smears over |q| rows.  The bank is a
 * third Doppler sum over the range map of the last process call, which de-chirps every pulse for each of K hypotheses of q,
 * walks the delay columns like the migration block above IN THE SAME SUM (two separate stages would each overwrite the
 * other), and keeps the strongest hypothesis per cell.  With the migration block's R, src, W, t and
 *   s(j,i)    = (int) rint( h[j] * (double) t(i) ), or 0 for every (j, i) when no migration table is set on the handle,
 *   q[k]        a BANK of K <= BLAH2HIP_MAX_RATES fp64 Doppler rates in BINS DRIFTED OVER THE CPI; positive: the Doppler rises
 *               through the CPI.  Chirp and walk are referenced to mid-CPI: the echo lands at its mid-CPI Doppler and delay,
 *   theta_k(i) = pi * q[k] * (double)(t(i) * t(i)) / (4.0 * n_doppler * n_doppler)             (fp64, on the host)
 *   c_k[i]    = ( (float) cos theta_k(i), (float) (-sin theta_k(i)) )                          (an fp32 table [K][n_doppler])
 *   M_k[j][d] = sum_i [0 <= d + s(j,i) < n_delay]  ( R[i][d + s(j,i)] c_k[i] ) W[(i src(j)) mod n_doppler]
 *   k*(j,d)   = the smallest k with the largest power p = x x + y y (fp32) of M_k[j][d]
 *   out[j][d] = M_k*[j][d],   index[j][d] = (uint8) k*
 * The arithmetic is walk_sum_kernel's (blah2hip_amb_migrate_dev's kernel body): fp32 complex multiply-adds in pulse order, a
 * block of 32 pulses summed on its own and added into a running sum, the range cell multiplied by the chirp first and by the twiddle second.  The order of the
 * additions depends on (j, k, i) alone: equal inputs give equal bits at every placement, every n_maps and for a hypothesis
 * at any position in the bank.  A candidate with q[k] == 0 in a ZERO-SHIFT row (rint(h[j] (n_doppler - 1)) == 0, or no table
 * set) is THE INPUT MAP'S CELL, bit for bit: it keeps what the hot-column and leak machinery wrote at the direct path; every
 * other candidate is the sum above.  So the bank {0} with no table returns the input maps, and the bank {0} with a table
 * returns blah2hip_amb_migrate_dev's maps (on maps without zero cells: c = (1, -0) may change the sign of a zero).  A term
 * whose column falls outside the map contributes zero.  The quadratic RANGE term of an acceleration is not modelled: it is
 * a t^2 / 2 = 1.25 m at 1 g and +-0.5 s, against a delay cell of 30 m or more. */
#define BLAH2HIP_MAX_RATES 16 /* hypotheses in a bank */
/* Host only: q = -accel * fc / 299792458 * T^2 with T = n_doppler * n_corr / fs; accel is the second derivative of the
 * bistatic range in m/s^2.  BLAH2HIP_ERR_INVALID: a NULL argument, fc not finite or not positive, accel not finite. */
int blah2hip_doppler_rate(blah2hip_amb_t h, double fc, double accel, double *q);
/* Builds the chirp table of the bank q[0 .. n_rates - 1] in fp64 on the host and copies it into a device buffer the handle
 * owns (allocated at the first call, freed by destroy; the call waits for the device, like blah2hip_amb_set_migration).
 * NULL or n_rates 0 clears the bank.  Duplicates are allowed; the lower index wins ties.  BLAH2HIP_ERR_INVALID, with the bank
 * that was set left as it was: n_rates above BLAH2HIP_MAX_RATES, an entry that is not finite, |q| above n_doppler (beyond
 * that the chirp's end frequency passes half the slow-time rate). */
int blah2hip_amb_set_rates(blah2hip_amb_t h, const double *q, uint32_t n_rates);
/* out, index and metrics for maps 0 .. n_maps - 1 of the handle's range map as the last process call left it:
 * blah2hip_amb_migrate_dev's contract throughout.  d_map: that call's map buffer (NULL = the handle's own), read only where
 * a candidate is the input cell.  d_out_map [n_maps][n_doppler][n_delay] may be the same pointer (in place) or a disjoint
 * buffer; d_out_index [n_maps][n_doppler][n_delay] uint8 may be NULL; d_out_metrics [n_maps][2] is Map::set_metrics of
 * every output map on the cells as written.  The migration table set on the handle at the time of the call is the walk.
 * Enqueues only -- walk_sum_kernel<4, 2> (BLAH2HIP_K_DOPPLER) and metrics_kernel (BLAH2HIP_K_METRICS) -- with no upload,
 * allocation or synchronisation, and can be captured in a graph.  The grid, ceil(n_delay / 64) ceil(n_doppler / 16)
 * workgroups per map (BLAH2HIP_INFO_RATE_GRID), depends on the geometry alone, never on n_maps; the bank goes in passes
 * inside a workgroup.  BLAH2HIP_ERR_INVALID, with nothing enqueued: every case of blah2hip_amb_migrate_dev but "no table
 * set"; no bank set; an index plane that overlaps a map or the metrics. */
int blah2hip_amb_rate_bank_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_maps, void *d_out_map, uint8_t *d_out_index,
                               double *d_out_metrics, void *stream);

/* ---- Integration along tracks (no reference counterpart: blah2 detects on single maps) ----
 * The integrator above sums a window of W CPIs IN THE SAME CELL.  Between CPIs an echo walks in delay (W times further than
 * inside one CPI, the migration block above) and, where it accelerates, climbs in Doppler (the rate bank above), so the
 * window sum of a fast or accelerating echo is a streak with a single look's level in every cell.  With tracks set, the
 * window sum is taken along the path an echo of each cell would have come, for a bank of Doppler-drift hypotheses, and the
 * strongest hypothesis is kept per cell.  p[c][j][d] = sum_k w_k |M_k[c][j][d]|^2 exactly as above (nci_power's fp32
 * arithmetic and order; c the CPI count, j the Doppler row, d the delay column).  With
 *   walk[j]   j = 0 .. n_doppler - 1: fp64 delay cells by which an echo in row j moves LATER per CPI (negative for an
 *             approaching target); any finite table,
 *   q[k]      k = 0 .. K - 1, K <= BLAH2HIP_MAX_RATES: fp64 Doppler rows the echo RISES per CPI (rows ascend in Doppler, as
 *             the handle's axis does),
 *   a         the age 0 .. W - 1: CPI g - a of the window that ends at g,
 * the tables are built in fp64 ON THE HOST and uploaded as int32 pairs [K][W][n_doppler]:
 *   r(k,a)    = (int) rint(q[k] * (double)a)
 *   jr(j,k,a) = j - r(k,a)                      no wrap: a row outside [0, n_doppler) contributes zero
 *   s(j,k,a)  = (int) rint(-0.5 * (double)a * (walk[j] + walk[jr]))    ties to even; the mean of the two rows' walks
 *   S_k[g][j][d] = sum_{a = W-1 .. 0, oldest first} [row valid][0 <= d+s < n_delay] p[g-a][jr][d+s]   fp32, __fadd_rn, from
 *                  the oldest valid term (a term that is left out adds +0, which changes no bit)
 *   k*  = 0 at the start; k replaces it only when S_k > S_k* (fp32 compare): the smallest k with the largest sum
 *   out[g][j][d] = ( sqrtf(scale * S_k*), 0 ),  index[g][j][d] = (uint8) k*,  scale = 1 / (W sum_k w_k) as above
 * a = 0 is the cell itself (s = 0, jr = j): an echo is reported at its position in the NEWEST CPI.  A term outside the map
 * contributes zero and scale does not change: cells near the edges are lower, as in walk_sum_kernel.  A NaN S_0 stays, with
 * index 0; a NaN S_k with k > 0 never wins (the compare is false).  A NaN or Inf cell of p reaches exactly the outputs whose
 * tracks pass through it.  With walk == 0 and the bank {0} the output maps are blah2hip_nci_process_dev's bit for bit (the
 * same additions in the same order); the metrics agree to 1e-3 dB only, because the partials' grid differs.  The error of a
 * cell against the fp64 value of the hypothesis the device names is the integrator's bound, (n_surv W + 8) 2^-24 of the cell:
 * all terms are non-negative and the selection adds no rounding.  Where two hypotheses lie closer than that, the device
 * may name either.
 * Statistics: under noise a cell is the largest of K Gamma(L) sums, L = n_surv W.  Make the detector with looks = L and
 * pfa / K (the union bound, as for the rate bank). */
#define BLAH2HIP_MAX_TRACK_SHIFT 1048576 /* the largest |s(j,k,a)| a table may hold, 2^20: the table is int32 and the kernel forms d + s in
                                          * int32, which cannot overflow below that (n_delay at or above 2^31 - 2^20 is refused too) */
/* Host only: the physical walk of the handle's own Doppler axis, walk[j] = -doppler[j] * n_corr * n_doppler * cpi_spacing / fc
 * for j = 0 .. n_doppler - 1 (evaluated left to right in fp64).  cpi_spacing: the distance between CPI starts in CPI lengths,
 * 1 for back-to-back CPIs.  BLAH2HIP_ERR_INVALID: a NULL argument, fc or cpi_spacing not finite or not positive. */
int blah2hip_nci_walk_table(blah2hip_amb_t amb, double fc, double cpi_spacing, double *walk);
/* Sets the tracks of an integrator: builds the (jr, s) tables from the HOST arrays walk [n_doppler] (NULL: all zero) and
 * q [n_rates] (NULL or n_rates 0: the bank {0}), uploads them, and allocates a ring of W - 1 + max_cpi fp32 planes of p,
 * indexed by g mod (W - 1 + max_cpi), in the place of the history planes.  max_cpi: the most CPIs one
 * blah2hip_nci_process_tracks_dev call will bring.  The call waits for the device (like blah2hip_amb_set_migration) and resets the
 * counter.  Duplicate rates are allowed; the lower index wins ties.  From then on the integrator refuses
 * blah2hip_nci_process_dev (its history lives in the ring); tracks cannot be cleared.
 * BLAH2HIP_ERR_INVALID, with what was set left as it was: a NULL handle, an entry that is not finite, n_rates above
 * BLAH2HIP_MAX_RATES, |q[k]| (W - 1) >= n_doppler, max_cpi == 0, n_surv * max_cpi above max_batch, a largest |s| above
 * BLAH2HIP_MAX_TRACK_SHIFT.  (BLAH2HIP_ERR_UNSUPPORTED: fewer metrics partials per map than track_sum_kernel has workgroups,
 * ceil(n_delay / 64) ceil(n_doppler / 8), one per 512 cells; no geometry the engine plans today.) */
int blah2hip_nci_set_tracks(blah2hip_nci_t n, const double *walk, const double *q, uint32_t n_rates, uint32_t max_cpi);
/* The next n_cpi CPIs along the tracks: blah2hip_nci_process_dev's contract throughout -- arguments, counting, n_out == 0 while
 * the window fills, enqueue only (no allocation, upload or synchronisation; can be captured in a graph), the same refusals
 * with nothing written and the counter unchanged -- with d_out_index [n_out][n_doppler][n_delay] uint8, the winning
 * hypothesis of every cell, which may be NULL.  blah2hip_nci_count and _reset work unchanged.
 * Two kernels: track_power_kernel (BLAH2HIP_NK_TRACK_POWER) reads every input cell once and writes p of the call's CPIs into
 * the ring; track_sum_kernel (BLAH2HIP_NK_TRACK_SUM) takes the window sums -- one launch for all n_out windows, reading the
 * (jr, s) pairs by scalar loads and the ring by 4-byte-per-lane loads at d + s -- and leaves one metrics partial per workgroup
 * and output map, which metrics_kernel folds in index order (no floating-point atomics).  The workgroups per CPI group and
 * per output map (BLAH2HIP_INFO_TRACK_GRID) depend on the geometry alone, never on n_cpi, the counter or n_out: outputs,
 * index and metrics are the same bits however the CPIs are cut into calls.
 * BLAH2HIP_ERR_INVALID in addition: no tracks set, n_cpi above the max_cpi of blah2hip_nci_set_tracks, an index plane that
 * overlaps a map or the metrics. */
int blah2hip_nci_process_tracks_dev(blah2hip_nci_t n, const void *d_map, uint32_t n_cpi, const float *w,
                                    void *d_out_map, uint8_t *d_out_index, double *d_out_metrics, uint32_t out_cap,
                                    uint32_t *n_out, uint64_t *first_end, void *stream);

/* ---- CfarDetector1D (CfarDetector1D.h:46-55) ---------------------------- */
/* dev: d_map/d_metrics as written by blah2hip_amb_process_dev (NULL = the
 * handle's internal buffers).  d_hits: [n_cpi][cap]; d_count: [n_cpi], zeroed
 * by the call.  Hits are appended in arbitrary order; count may exceed cap
 * (then only cap were stored). */
int blah2hip_cfar1d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics,
                        uint32_t n_cpi, double pfa, int32_t n_guard, int32_t n_train,
                        int32_t min_delay, double min_doppler, blah2hip_hit_t *d_hits,
                        uint32_t cap, uint32_t *d_count, void *stream);
/* Builds the threshold table alpha[n] = n (pfa^(-1/n) - 1) (BLAH2HIP_OPT_CFAR_LOOKS above 1: blah2hip_cfar_alpha's for
 * the option's value at this call) for this (pfa, n_train) ahead of
 * time (one blocking upload).  blah2hip_cfar1d_dev does it on the first call with a new
 * tuple and only enqueues afterwards.  A table built by *_prepare stays resident for the handle's lifetime (a graph
 * captured after it may replay at any time); the tables the dev calls build on their own are a cache of eight, least
 * recently used first out. */
int blah2hip_cfar1d_prepare(blah2hip_amb_t h, double pfa, int32_t n_train);
/* The detectors' threshold factors for cells that are sums of `looks` looks (the output maps of blah2hip_nci_process_dev:
 * looks = n_surv * window), what BLAH2HIP_OPT_CFAR_LOOKS makes the tables from.  Host arithmetic only: no GPU is touched.
 * alpha[n], n = 1 .. max_n, for the threshold alpha[n] * (tot / n) over n training cells; alpha[0] = NaN (a cell without
 * training cells never exceeds); alpha: max_n + 1 doubles.  Under noise a cell of the sum is Gamma(L) and the training sum
 * Gamma(nL); with t = alpha / n and m = nL
 *   Pfa(t) = sum_{k=0}^{L-1} C(m+k-1, k) t^k / (1+t)^(m+k)
 * looks == 1: (1+t)^-n, solved in closed form: n (pfa^(-1/n) - 1) with the libm pow the reference calls
 * (CfarDetector1D.cpp:76), bit for bit what the detectors have always tabulated, for any pfa.  looks > 1: Pfa(t) = pfa by
 * bisection in fp64 until the interval no longer splits, Pfa evaluated term by term in the log domain (no lgamma); the
 * result back-substitutes to pfa within 1e-10 of it.  The one-look factor on a sum of L looks is far too high: at L = 4,
 * n = 8, pfa = 1e-3 it is 10.97 where 3.824 holds the pfa -- 4.6 dB of sensitivity.
 * BLAH2HIP_ERR_INVALID: a NULL table, looks outside [1, BLAH2HIP_MAX_CFAR_LOOKS], pfa outside (0, 1) with looks > 1. */
int blah2hip_cfar_alpha(double pfa, uint32_t looks, uint32_t max_n, double *alpha);
/* host: runs the detector on CPI `cpi` of the handle's internal map and
 * returns Detection's three vectors (delay bins, Doppler Hz, snr) in the
 * reference's emission order (row-major, CfarDetector1D.cpp:36-92). */
int blah2hip_cfar1d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, int32_t n_guard,
                            int32_t n_train, int32_t min_delay, double min_doppler, double *delay,
                            double *doppler, double *snr, uint32_t cap, uint32_t *count);

/* The same detector on a map held by the HOST (any Map<complex<double>>, e.g. one the caller
 * modified or built itself): complex fp32 cells [n_doppler][n_delay], Map::delay (bins),
 * Map::doppler (Hz) and Map::noisePower.  Uploads, runs the GPU kernel on `device`, frees. */
int blah2hip_cfar1d_map(const float *map, uint32_t n_doppler, uint32_t n_delay, const int32_t *delay_axis,
                        const double *doppler_axis, double noise_power, double pfa, int32_t n_guard,
                        int32_t n_train, int32_t min_delay, double min_doppler, int device, double *delay,
                        double *doppler, double *snr, uint32_t cap, uint32_t *count);

/* 2-D cell-averaging CFAR (BASELINE.json configs[2]; NOT in the reference, which
 * only has the 1-D detector).  Extension defined in SURVEY.md section 8g: training
 * rectangle (2(ngd+ntd)+1) x (2(ngf+ntf)+1) minus the guard box, in-bounds cells
 * only, delay column 0 never trains, |z|^2 statistic, alpha = N(pfa^(-1/N)-1);
 * with n_guard_doppler = n_train_doppler = 0 it is exactly blah2hip_cfar1d_*.
 * Same output conventions as the 1-D entry points.
 * Cells that are not finite: |z|^2 is formed in fp64, and a NaN or +Inf cell makes the window sums that hold it NaN
 * or +Inf.  The one-pass kernels (stream, tile) sum every window on its own, so exactly the cells whose training
 * window holds such a cell are lost (nothing exceeds a NaN or +Inf threshold), and a +Inf cell itself is reported when
 * its own window is finite.  The summed-area table carries the value into every prefix below and right of the cell:
 * there the table kernels may lose detections (all of them, in the worst case), but they never report a cell the
 * one-pass kernels would not. */
int blah2hip_cfar2d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi,
                        double pfa, int32_t n_guard_delay, int32_t n_train_delay,
                        int32_t n_guard_doppler, int32_t n_train_doppler, int32_t min_delay,
                        double min_doppler, blah2hip_hit_t *d_hits, uint32_t cap, uint32_t *d_count,
                        void *stream);
/* Builds the threshold table for this parameter tuple and, for windows beyond the one-pass tile kernel's
 * halo (see BLAH2HIP_OPT_CFAR2D_KERNEL), allocates the summed-area table ([max_batch][nD+1][nDelay+1]
 * doubles); blah2hip_cfar2d_dev calls it implicitly. */
int blah2hip_cfar2d_prepare(blah2hip_amb_t h, double pfa, int32_t n_guard_delay, int32_t n_train_delay,
                            int32_t n_guard_doppler, int32_t n_train_doppler);
int blah2hip_cfar2d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, int32_t n_guard_delay,
                            int32_t n_train_delay, int32_t n_guard_doppler, int32_t n_train_doppler,
                            int32_t min_delay, double min_doppler, double *delay, double *doppler,
                            double *snr, uint32_t cap, uint32_t *count);

/* ---- Ordered-statistic CFAR (OS-CFAR, Rohling; NOT in the reference) -------
 * The detectors above average their training cells; a second echo, a clutter edge or a sidelobe inside the training window
 * raises that mean and masks the cell under test.  Here the threshold is alpha[n] * x_(k), the k-th smallest of the n
 * in-bounds training cells: a handful of interferers in the window do not move it.  With p = |z|^2 formed in fp64 as the
 * detectors above form it, training cells p_1 .. p_n of the cell under test c, and
 *   k(n) = max(1, ceil(n * rank_permille / 1000))                 integer arithmetic, rank_permille in 1 .. 1000
 *   hit  <=>  n >= 1  and  #{ i : alpha[n] * p_i < p_c } >= k(n)   product and compare in fp64
 * This is p_c > alpha[n] * x_(k) (multiplying by a positive factor and rounding is monotone) stated as a count: no sort.
 * The rule is the contract and fixes the special values: a NaN or +Inf training cell is never below (it costs its window
 * one rank, not the detection), a NaN cell under test never hits, a +Inf cell hits when k of its training cells are finite,
 * an all-zero map has no hits.  |z|^2 of fp32 parts has exact products in fp64 and rounds once, alpha * p_i is one
 * multiply: the decision is the same bits on the device and in an fp64 restatement with the same table (process.py:
 * oscfar_hits).
 *
 * blah2hip_oscfar_alpha: the tables, host arithmetic only (no GPU is touched).  alpha[0] = NaN, rank[0] = 0; for
 * n = 1 .. max_n rank[n] = k(n) and alpha[n] solves Pfa(alpha; n, k) = pfa for cells that are sums of `looks` looks of noise:
 *   looks == 1:  Pfa = prod_{i=0}^{k-1} (n - i) / (n - i + alpha), solved by bisection on its logarithm
 *                -sum log1p(alpha / (n - i)) until the interval no longer splits (its upper end);
 *   looks = L > 1 (the maps of blah2hip_nci_process_dev, Gamma(L) cells):
 *                Pfa = int f_(k)(x) Q_L(alpha x) dx,  Q_L(t) = e^-t sum_{j<L} t^j / j!,
 *                f_(k)(x) = n! / ((k-1)! (n-k)!) P^(k-1) Q_L(x)^(n-k) x^(L-1) e^-x / (L-1)!,  P = 1 - Q_L(x),
 *                the density of the k-th smallest of n Gamma(L) variables; composite Simpson, 16384 intervals over the
 *                interval on which the integrand is within e^-60 of its largest value.  alpha: the bracket [hi / 2, hi] by
 *                doubling (every trial on an interval of its own), then the same bisection on the interval of the
 *                bracket's lower end, which holds the integrand of every larger alpha.
 * alpha: max_n + 1 doubles; rank: max_n + 1 words, or NULL.  BLAH2HIP_ERR_INVALID: a NULL table, looks outside
 * [1, BLAH2HIP_MAX_CFAR_LOOKS], rank_permille outside [1, 1000], pfa outside (0, 1). */
int blah2hip_oscfar_alpha(double pfa, uint32_t looks, uint32_t rank_permille, uint32_t max_n, double *alpha, uint32_t *rank);
/* The 1-D detector: geometry, quirks and output conventions of blah2hip_cfar1d_dev / _prepare / _process (leading cells
 * never train on delay column 0, min_delay / min_doppler skips, count may exceed cap, row-major emission order of _process),
 * n_train up to 127.  The tables (alpha and rank, uploaded together) are made for the handle's BLAH2HIP_OPT_CFAR_LOOKS at
 * the time of the call and live in a cache of their own keyed by (pfa, looks, rank_permille, size) with the rules of the
 * averaging detectors' cache (eight entries, least recently used first out, _prepare pins), which these calls do not touch:
 * _dev only enqueues after the first call with a new tuple.  Timing counts under BLAH2HIP_K_CFAR. */
int blah2hip_oscfar1d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi, double pfa,
                          uint32_t rank_permille, int32_t n_guard, int32_t n_train, int32_t min_delay, double min_doppler,
                          blah2hip_hit_t *d_hits, uint32_t cap, uint32_t *d_count, void *stream);
int blah2hip_oscfar1d_prepare(blah2hip_amb_t h, double pfa, uint32_t rank_permille, int32_t n_train);
int blah2hip_oscfar1d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, uint32_t rank_permille, int32_t n_guard,
                              int32_t n_train, int32_t min_delay, double min_doppler, double *delay, double *doppler,
                              double *snr, uint32_t cap, uint32_t *count);
/* The 2-D detector on the window of blah2hip_cfar2d_*: the rectangle minus the guard box, in-bounds cells only, delay
 * column 0 never trains; with n_guard_doppler = n_train_doppler = 0 it reports the 1-D detector's hits.  One kernel with a
 * tile and its halo in LDS: n_guard_doppler + n_train_doppler <= 24 and n_guard_delay + n_train_delay <= 40; a wider window
 * is BLAH2HIP_ERR_UNSUPPORTED (a rank has no summed-area form).  BLAH2HIP_OPT_CFAR2D_KERNEL does not apply. */
int blah2hip_oscfar2d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi, double pfa,
                          uint32_t rank_permille, int32_t n_guard_delay, int32_t n_train_delay, int32_t n_guard_doppler,
                          int32_t n_train_doppler, int32_t min_delay, double min_doppler, blah2hip_hit_t *d_hits,
                          uint32_t cap, uint32_t *d_count, void *stream);
int blah2hip_oscfar2d_prepare(blah2hip_amb_t h, double pfa, uint32_t rank_permille, int32_t n_guard_delay,
                              int32_t n_train_delay, int32_t n_guard_doppler, int32_t n_train_doppler);
int blah2hip_oscfar2d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, uint32_t rank_permille, int32_t n_guard_delay,
                              int32_t n_train_delay, int32_t n_guard_doppler, int32_t n_train_doppler, int32_t min_delay,
                              double min_doppler, double *delay, double *doppler, double *snr, uint32_t cap,
                              uint32_t *count);

/* ---- Greatest-of and smallest-of CFAR (GO-CFAR, Hansen and Sawyers; SO-CFAR, Trunk; NOT in the reference) -------
 * The averaging detectors take one mean over both sides of the cell under test.  At a clutter edge -- the end of the clutter
 * filter's lag span, the flank of the direct-path residue -- half of the window lies in the weak region, the mean is too low
 * and the cells just inside the strong region are reported as noise; greatest-of thresholds against the larger half.  Two
 * echoes in each other's window raise each other's mean; smallest-of thresholds against the smaller half, one of which is
 * clean (the ordered-statistic detectors do that at several times the cost).  With p = re^2 + im^2 in fp64 from the fp32
 * parts, formed as the detectors above form it, and kind BLAH2HIP_CFAR_GO or BLAH2HIP_CFAR_SO:
 *
 * 1-D, geometry and quirks of blah2hip_cfar1d_*.  For cell (i, j) of a row with nC delay bins
 *   leading set  A = { k : j - nG - nT <= k < j - nG,  0 < k < nC }      (delay column 0 never trains)
 *   lagging set  B = { k : j + nG < k <= j + nG + nT,  0 <= k < nC }
 *   a = |A|, b = |B|;  S_A, S_B: fp64 sums started at 0.0 and taken in ascending k;  mu_A = S_A / (double)a, mu_B = S_B / (double)b
 *   a >= 1 and b >= 1, alpha = alpha(kind; a, b):   GO hits  <=>  p_c > alpha mu_A  and  p_c > alpha mu_B
 *                                                   SO hits  <=>  p_c > alpha mu_A  or   p_c > alpha mu_B
 *     each threshold one fp64 multiply and one compare; no max or min is formed.  The rule is the contract and fixes the
 *     special values: a NaN half never supports a hit, a NaN cell under test never hits, an all-zero map has no hits.
 *   exactly one half empty: the cell-averaging rule over the other,  p_c > alpha_ca[a + b] (S / (a + b)),  alpha_ca
 *     blah2hip_cfar_alpha's one-look value;   both empty: no hit.
 * The min_delay / min_doppler skips, the hit records, snr = 5 log10(p_c) - noisePower, the count > cap behaviour and the
 * emission order of _process are those of blah2hip_cfar1d_*.
 *
 * 2-D: the halves are split along delay and each is averaged over the window's Doppler extent, n_rows_doppler = hR rows on
 * either side.  Rows [i - hR, i + hR] in [0, nD); leading columns [j - nGd - nTd, j - nGd - 1] in [1, nC); lagging columns
 * [j + nGd + 1, j + nGd + nTd] in [0, nC); the columns j - nGd .. j + nGd train in no row (the cell's own Doppler sidelobes
 * stay out of both halves).  a = rows colsLeading, b = rows colsLagging.  The sums have a fixed order, so the decision is
 * reproducible bit for bit: per column C[k] = sum of p[ii][k] over the rows in ascending ii, started at 0.0, then S = sum of
 * C[k] in ascending k, started at 0.0 -- no sliding add-and-subtract and no summed-area table (different bits, and small
 * windows lost beside tall cells).  With hR = 0 the detector reports exactly the 1-D detector's hits.  hR <= 24 and
 * nGd + nTd <= 40; a wider window is BLAH2HIP_ERR_UNSUPPORTED.
 *
 * Threshold factors, one look.  Under noise of unit power the cell is Exp(1), U = Gamma(a) / a, V = Gamma(b) / b, and
 *   T(alpha; a, b) = E[e^(-alpha U); U < V] = sum_{j=0}^{b-1} C(a-1+j, j) (b/a)^j s^-(a+j),   s = 1 + (alpha + b) / a
 *   Pfa_SO(alpha; a, b) = T(alpha; a, b) + T(alpha; b, a)
 *   Pfa_GO(alpha; a, b) = (1 + alpha/a)^-a + (1 + alpha/b)^-b - Pfa_SO(alpha; a, b)
 *                       = T'(alpha; a, b) + T'(alpha; b, a),   T' the series of T from j = b on (the whole series sums to
 *                         (1 + alpha/a)^-a): this form is the one evaluated, positive terms until what is left is below
 *                         1e-17 of the sum -- with uneven halves and a small pfa the difference above loses eight digits
 * T term by term in the log domain (the ratio of consecutive terms is ((a-1+j)/j) (b/a) / s); for a = b = n it is the textbook
 * 2 sum_k C(n-1+k, k) (2 + alpha/n)^-(n+k).  alpha solves Pfa = pfa by bisection in fp64 until the interval no longer splits
 * (its upper end), after bracketing by doubling, and back-substitutes to pfa within 1e-10 of it; alpha(a, b) = alpha(b, a).
 * pfa 1e-3: alpha_GO(8, 8) = 7.487313, alpha_SO(8, 8) = 12.599715 (averaging over the 16: 8.638824); alpha_GO(3, 8) =
 * 8.211435, alpha_SO(3, 8) = 27.069698; alpha_GO(1, 1) = (-3 + sqrt(8001)) / 2, alpha_SO(1, 1) = 1998.
 * blah2hip_gocfar_alpha: host arithmetic only (no GPU is touched): alpha[i] for the pair (a[i], b[i]), i < n_pairs; a pair
 * with one zero gets the averaging value of the other half, the pair (0, 0) NaN.  BLAH2HIP_ERR_INVALID: a NULL pointer, an
 * unknown kind, pfa outside (0, 1).
 *
 * The entry points take their averaging detector's arguments with `kind` after pfa (the 2-D ones n_rows_doppler in the place
 * of the two Doppler sizes; _prepare takes n_guard too, because the table holds the pairs the map's geometry reaches under
 * the window).  The tables live in a cache of their own keyed by (pfa, kind, window) for the handle's map geometry, with the
 * rules of the averaging detectors' cache (eight unpinned entries, least recently used first out, _prepare pins, a miss
 * while the stream is being captured is refused), which these calls do not touch.  Timing counts under BLAH2HIP_K_CFAR.
 * The factors are made for one look per cell: a call while BLAH2HIP_OPT_CFAR_LOOKS is above 1 is BLAH2HIP_ERR_UNSUPPORTED
 * (the Gamma(L) form is a double sum whose cost does not fit a table build).  Every refusal writes nothing. */
#define BLAH2HIP_CFAR_GO 1
#define BLAH2HIP_CFAR_SO 2
int blah2hip_gocfar_alpha(double pfa, uint32_t kind, uint32_t n_pairs, const uint32_t *a, const uint32_t *b, double *alpha);
int blah2hip_gocfar1d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi, double pfa, uint32_t kind,
                          int32_t n_guard, int32_t n_train, int32_t min_delay, double min_doppler, blah2hip_hit_t *d_hits,
                          uint32_t cap, uint32_t *d_count, void *stream);
int blah2hip_gocfar1d_prepare(blah2hip_amb_t h, double pfa, uint32_t kind, int32_t n_guard, int32_t n_train);
int blah2hip_gocfar1d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, uint32_t kind, int32_t n_guard, int32_t n_train,
                              int32_t min_delay, double min_doppler, double *delay, double *doppler, double *snr, uint32_t cap,
                              uint32_t *count);
int blah2hip_gocfar2d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi, double pfa, uint32_t kind,
                          int32_t n_guard_delay, int32_t n_train_delay, int32_t n_rows_doppler, int32_t min_delay,
                          double min_doppler, blah2hip_hit_t *d_hits, uint32_t cap, uint32_t *d_count, void *stream);
int blah2hip_gocfar2d_prepare(blah2hip_amb_t h, double pfa, uint32_t kind, int32_t n_guard_delay, int32_t n_train_delay,
                              int32_t n_rows_doppler);
int blah2hip_gocfar2d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, uint32_t kind, int32_t n_guard_delay,
                              int32_t n_train_delay, int32_t n_rows_doppler, int32_t min_delay, double min_doppler,
                              double *delay, double *doppler, double *snr, uint32_t cap, uint32_t *count);

/* ---- Clutter-map CFAR (Nitzberg; NOT in the reference) and the gate behind the spatial detectors -------
 * The detectors above compare a cell with its neighbours in the same map, so whatever stands out from its surroundings
 * is reported in every CPI: a clutter discrete the filter left, the direct path's residue, an interferer's Doppler line.
 * Here a cell is thresholded against an exponentially weighted average b of its OWN past power: a cell that is always
 * bright is never reported, an echo that moves through cells is.  Per CPI c of a call, in time order, for every cell:
 *   p = fmaf(re, re, im * im)                     fp32, nci_power's form
 *   u = p * s[c]  with BLAH2HIP_CMAP_NORMALISE,   s[c] = (float) exp10(-noisePower[c] / 5) formed in fp64 from
 *                                                 d_metrics[c][0]; noisePower is the mean of 10 log10|z|, so s is one over
 *                                                 the squared geometric-mean amplitude of the map: the illuminator's
 *                                                 content moves the whole map's level from CPI to CPI, and u is what is
 *                                                 stationary.  Without the flag u = p.
 *   a = a0 + c                                    the map's age: the CPIs it has absorbed since create or reset (a0: a
 *                                                 host counter across calls)
 *   exceeds  <=>  a >= 1  and  (double)u > alpha[min(a, 16 T)] * (double)b        product and compare in fp64
 *   then, hit or not:  k = min(a + 1, T),  r = 1.f / (float)k (fp32 division),
 *                      b = u at a == 0,  b = fmaf(r, u - b, b) otherwise
 * -- the running mean of the first T CPIs, the exponential average of weight 1 / T after them: at every age the estimate
 * of the lowest variance, with a threshold factor that is exact at every age.  T is the memory, 1 ..
 * BLAH2HIP_MAX_CMAP_MEMORY.  A cell whose u is NaN or +-Inf neither exceeds nor updates.  At a == 0 the plane's old content
 * is not read (reset clears nothing); a cell that is not finite then starts from b = 0.  An all-zero map has no exceeding
 * cell (0 > alpha * 0 is false).
 * A cell that exceeds is a HIT when it passes the min_delay / min_doppler skips of blah2hip_cfar1d_dev (the same row and
 * delay tests), with snr = 5 log10(p) - noisePower[c] as there; hits are appended through d_count[c] in arbitrary order and
 * the count may exceed cap.  The optional plane d_out_exceed [n_cpi][n_doppler][n_delay] of uint8 gets 1 where the cell
 * exceeds and 0 elsewhere, skips or not.  d_out_level [n_cpi] floats, when not NULL, gets s[c] (1 without the flag), so
 * that a restatement can be fed the device's own factor.
 *
 * Thresholds.  Under noise u is exponential and b = sum_i c_i u_i over independent past values, so
 *   Pfa(alpha) = prod_i 1 / (1 + alpha c_i).
 * The weights at age a:  a <= T: a times 1 / a, which gives alpha = a (pfa^(-1/a) - 1), blah2hip_cfar_alpha's one-look
 * value for n = a;  a > T: w (1 - w)^m for m = 0 .. a - T - 1 and T times (1 - w)^(a - T) / T, with w = 1 / T.
 * blah2hip_cmap_alpha: host arithmetic only (no GPU is touched).  alpha[0] = NaN; alpha[a], a = 1 .. max_age, solves
 * Pfa = pfa by bisection on -sum log1p(alpha c_i) until the interval no longer splits (its upper end); entries beyond 16 T
 * repeat the one at 16 T (the difference to the entry before it is below 1.5e-14 there for T = 4 .. 64).  alpha:
 * max_age + 1 doubles.  pfa = 1e-2, T = 8: alpha[1 .. 8] = 99, 18, 10.9248, 8.6491, 7.5594, 6.9266, 6.5149, 6.2262,
 * alpha[16] = 5.45031, alpha[128] = 5.33810.  BLAH2HIP_ERR_INVALID: a NULL table, memory outside
 * [1, BLAH2HIP_MAX_CMAP_MEMORY], pfa outside (0, 1).
 * Error of b against the same recursion in fp64 (u from the fp32 cells and the device's s[c] in fp64, r the fp32 quotient):
 * with eps = 2^-24 and U the largest u the cell has absorbed, u arrives with 3 eps U (two roundings in p, one with the
 * level) and enters with weight r, the difference u - b rounds once (eps U, weight r), the fma's result once (eps U), and
 * the step damps the error e that is there by 1 - r:  e' <= (1 - r) e + (4 r + 1) eps U.  From e = 3 eps U at a == 0 this
 * gives, by induction over the steps (k never falls),  |b - b_fp64| <= (k + 4) 2^-24 U,  k = min(a, T) after a CPIs.
 * Integrated maps (more than one look per cell) are not built: a call while the ambiguity handle's
 * BLAH2HIP_OPT_CFAR_LOOKS is above 1 is BLAH2HIP_ERR_UNSUPPORTED. */
#define BLAH2HIP_MAX_CMAP_MEMORY 64
#define BLAH2HIP_CMAP_NORMALISE 1 /* flag of blah2hip_cmap_create: u = p * s[c] */
typedef struct blah2hip_cmap_s *blah2hip_cmap_t;
int blah2hip_cmap_alpha(double pfa, uint32_t memory, uint32_t max_age, double *alpha);
/* A clutter map for the maps of `amb` (its geometry), age 0; allocates the plane b, 4 bytes a cell.
 * BLAH2HIP_ERR_INVALID: a NULL argument, memory outside [1, BLAH2HIP_MAX_CMAP_MEMORY], unknown flag bits. */
int blah2hip_cmap_create(blah2hip_amb_t amb, uint32_t memory, uint32_t flags, blah2hip_cmap_t *out);
/* Waits for the device (enqueued calls use the plane and the tables) and frees them.  Call it BEFORE blah2hip_amb_destroy
 * of its handle. */
int blah2hip_cmap_destroy(blah2hip_cmap_t cm);
/* Age 0: the next CPI starts the average anew.  Host only, enqueues nothing (calls enqueued earlier are not affected). */
int blah2hip_cmap_reset(blah2hip_cmap_t cm);
/* *age: the CPIs absorbed since the creation or the last reset (the calls enqueued so far included). */
int blah2hip_cmap_age(blah2hip_cmap_t cm, uint64_t *age);
/* Builds and uploads alpha[0 .. 16 T] for this pfa ahead of time (blocking).  blah2hip_cmap_process_dev does it on the first
 * call with a new pfa and only enqueues afterwards; the tables follow the rules of the detectors' cache (eight per clutter
 * map, least recently used first out, a table built by _prepare stays for the handle's lifetime). */
int blah2hip_cmap_prepare(blah2hip_cmap_t cm, double pfa);
/* The next n_cpi CPIs.  d_map / d_metrics as blah2hip_cfar1d_dev takes them (NULL = the ambiguity handle's internal
 * buffers).  d_hits [n_cpi][cap] and d_count [n_cpi] (zeroed by the call) may BOTH be NULL for gate-only use;
 * d_out_exceed and d_out_level may be NULL.  One kernel (cmap_kernel; timing counts under BLAH2HIP_K_CFAR) reads every
 * map cell once, reads b at its start (not at age 0) and writes it once at its end: 8 n_cpi + 8 bytes a cell and call, and
 * n_cpi more with the exceed plane.  The bits of b, of the exceed planes and of the levels, and the hit sets, do not
 * depend on how the CPIs were cut into calls.  Calls on one clutter map must be ordered on the device.
 * The age lives in the launch arguments and is counted on the host, so the call only enqueues and can be captured in a
 * graph -- a replay repeats the launch, not the count.
 * BLAH2HIP_ERR_INVALID, with nothing enqueued and the age and the plane as they were: a NULL handle, n_cpi outside
 * [1, max_batch], pfa outside (0, 1), exactly one of d_hits / d_count NULL, cap == 0 with a list, a map that is not
 * 8-byte aligned. */
int blah2hip_cmap_process_dev(blah2hip_cmap_t cm, const void *d_map, const double *d_metrics, uint32_t n_cpi, double pfa,
                              int32_t min_delay, double min_doppler, blah2hip_hit_t *d_hits, uint32_t cap, uint32_t *d_count,
                              uint8_t *d_out_exceed, float *d_out_level, void *stream);
/* The gate: d_hits_out [n_cpi][cap] gets the records of d_hits [n_cpi][cap] whose cell has a non-zero byte in d_exceed
 * [n_cpi][n_doppler][n_delay], in their order (a stable compaction, one workgroup per CPI: hits_gate_kernel), and
 * d_count_out [n_cpi] their number.  A count beyond cap means the first cap records are the list; a record outside the map
 * is dropped.  BLAH2HIP_ERR_INVALID: a NULL argument, n_cpi outside [1, max_batch], cap == 0, an output that overlaps its
 * input (the compaction cannot run in place). */
int blah2hip_cmap_gate_dev(blah2hip_cmap_t cm, const uint8_t *d_exceed, uint32_t n_cpi, const blah2hip_hit_t *d_hits,
                           uint32_t cap, const uint32_t *d_count, blah2hip_hit_t *d_hits_out, uint32_t *d_count_out,
                           void *stream);
/* Waits for the device and downloads b: [n_doppler][n_delay] floats (zero before the first CPI). */
int blah2hip_cmap_read_background(blah2hip_cmap_t cm, float *b);

/* ---- Centroid / Interpolate (host-side, tens of detections) -------------- */
/* Centroid::process (src/process/detection/Centroid.cpp:19-73): keeps a
 * detection unless a stronger one lies strictly inside its
 * (+-n_delay bins, +-n_doppler*resolution Hz) box.  The box's delay limits are
 * uint16_t in the reference (they wrap for delay - n_delay < 0); reproduced.
 * In/out arrays may not alias.  *count_out <= count. */
int blah2hip_centroid(const double *delay, const double *doppler, const double *snr, uint32_t count,
                      uint16_t n_delay, uint16_t n_doppler, double resolution_doppler,
                      double *delay_out, double *doppler_out, double *snr_out, uint32_t *count_out);
/* Interpolate::process (src/process/detection/Interpolate.cpp:20-91): 3-point
 * quadratic peak interpolation in delay and/or Doppler on the map cells
 * (complex fp32, [n_doppler][n_delay]); drops detections on the map edge or
 * whose neighbours are stronger.  The Doppler branch stores its SNR estimate
 * into the delay variable like the reference does (:80). */
int blah2hip_interpolate(const double *delay, const double *doppler, const double *snr, uint32_t count,
                         const float *map, uint32_t n_doppler, uint32_t n_delay, const int32_t *delay_axis,
                         const double *doppler_axis, double noise_power, int do_delay, int do_doppler,
                         double *delay_out, double *doppler_out, double *snr_out, uint32_t *count_out);

/* ---- Centroid + Interpolate on the device (blah2.cpp:285-287) -------------
 * Centroid::process (Centroid.cpp:19-73), then Interpolate::process (Interpolate.cpp:20-91) on its survivors, for
 * n_cpi device-resident hit lists as blah2hip_cfar1d_dev / blah2hip_cfar2d_dev leave them (d_hits [n_cpi][cap],
 * d_count [n_cpi]; a count beyond cap: the first cap records are the list, d_count is not written) and the maps they
 * came from (d_map / d_metrics as for the detectors, NULL = the handle's internal buffers).  The same arithmetic as
 * blah2hip_centroid and blah2hip_interpolate on the handle's own axes: delay = col + delay[0], doppler = doppler[row];
 * the uint16_t delay limits, the strict inequalities, the Doppler estimate stored into the delay variable (:80) and
 * max(max(.,.),.) of :86 included.  do_centroid = 0 skips the first step, do_delay / do_doppler are
 * Interpolate's two flags (both 0: the list after Centroid).  A record whose row or col lies outside the map is ignored.
 * d_out: [n_cpi][cap_out] records in arbitrary order; d_count_out [n_cpi]: the number of final detections, also when it
 * exceeds cap_out (then only cap_out were stored).  Enqueues ONE kernel on `stream` and nothing else: neither output
 * needs to be zeroed.  Calls on one handle must be ordered on the device (one stream, or events): the multi-workgroup form
 * counts through words the handle owns.  n_cpi outside [1, max_batch], cap == 0 or a NULL list / count / output:
 * BLAH2HIP_ERR_INVALID. */
int blah2hip_detect_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi,
                        const blah2hip_hit_t *d_hits, uint32_t cap, const uint32_t *d_count,
                        uint16_t n_centroid_delay, uint16_t n_centroid_doppler, double resolution_doppler,
                        int do_centroid, int do_delay, int do_doppler,
                        blah2hip_det_t *d_out, uint32_t cap_out, uint32_t *d_count_out, void *stream);

/* ---- WienerHopf clutter filter (WienerHopf.h:68-78) ---------------------
 * nBins = delay_max - delay_min taps (WienerHopf.cpp:12).  Up to 4081 taps run on one on-chip transform (fp32 planes or the int16
 * words).  More ("long" filters, round 6): the same kernels chunk by chunk of 2048 lags / taps on rotated and shifted copies of the
 * channels, the Toeplitz solve by one workgroup on vectors in global memory -- fp32 planes only (BLAH2HIP_FMT_I16: ERR_UNSUPPORTED),
 * no blah2hip_clutter_set_option; built for coverage, not speed (2 nChunks - 1 correlation passes, nChunks FIR passes, a few
 * microseconds per order of the solve).  nBins > n_samples: ERR_UNSUPPORTED (the reference reads its n_samples correlation lags out
 * of bounds there, WienerHopf.cpp:76-108). */
int blah2hip_clutter_create(int32_t delay_min, int32_t delay_max, uint32_t n_samples, int device,
                            uint32_t max_batch, blah2hip_clutter_t *out);
/* Taps per BLOCK of the CPI (the batched filter, ECA-B): the CPI is cut into n_blocks blocks of L = n_samples / n_blocks, the taps
 * are estimated per block and the filter's history runs on across the block edges.  n_blocks = 1 is blah2hip_clutter_create (the
 * same code path, the same bits).  With n_blocks > 1, block j of CPI c is VIRTUAL CPI v = c * n_blocks + j:
 *   estimation:  r_v, b_v, ok_v, w_v are what the filter computes on the L samples x[jL .. (j+1)L), y[jL .. (j+1)L) taken alone
 *                (shift by delayMin and correlations circular inside the block: a true autocorrelation Toeplitz matrix);
 *   application: xs[i] = x[(i - delayMin) mod n_samples] over the WHOLE CPI (uint32 arithmetic, xs[m < 0] = 0), and for n in
 *                block j  y_out[n] = y[n] - sum_k w_v[k] xs[n - k]: the history of block j > 0 is the samples of block j - 1,
 *                only block 0 sees the zero fill;
 *   a block with ok_v = 0 passes y through (the dev entry points), the other blocks are still filtered; the host entry points
 *   return the AND over the blocks in *ok and do not write y_out when it is 0.
 * The plan (transform length, correlation form, segments, grids; blah2hip_clutter_get_dims, _set_option, _get_info) is made for a
 * CPI of L samples and a batch of max_batch * n_blocks.  d_ok ([n_cpi * n_blocks]), blah2hip_clutter_read_last,
 * blah2hip_clutter_taps_dev ([n_cpi * n_blocks][n_bins]), blah2hip_clutter_solve(_dev) and the solve's info count virtual CPIs;
 * blah2hip_clutter_estimate_dev_fmt leaves the per-block taps.  The FIR reads every window whole: BLAH2HIP_CLUTTER_INFO_FIR_CARRY
 * reports 0.  d_y_out may alias d_y (FMT_C32).  The timing slots are the same four.
 * BLAH2HIP_ERR_INVALID: n_blocks == 0, n_samples % n_blocks != 0.  BLAH2HIP_ERR_UNSUPPORTED with n_blocks > 1: L < delay_max -
 * delay_min (the reference reads out of bounds on such a block), a long filter (more than 4081 taps), and
 * blah2hip_clutter_process_multi_dev_fmt on such a handle.  The range kernel's fused FIR takes one tap set per CPI: a chain with
 * blocks runs the two-stage filter. */
int blah2hip_clutter_create_ex(int32_t delay_min, int32_t delay_max, uint32_t n_samples, uint32_t n_blocks, int device,
                               uint32_t max_batch, blah2hip_clutter_t *out);
int blah2hip_clutter_destroy(blah2hip_clutter_t h);
/* host: y_out = y - w*x (WienerHopf.cpp:156-160); *ok = 0 when the normal
 * equations are not positive definite (the reference returns false and the CPI
 * is skipped, blah2.cpp:270-273), in which case y_out is not written. */
int blah2hip_clutter_process_c64(blah2hip_clutter_t h, const double *x, const double *y, uint32_t n,
                                 double *y_out, int *ok);
int blah2hip_clutter_process_c32(blah2hip_clutter_t h, const float *x, const float *y, uint32_t n,
                                 float *y_out, int *ok);
/* dev: complex fp32 planes resident in HBM; d_y_out may alias d_y.
 * d_ok: [n_cpi] int32 flags.  Enqueues only. */
int blah2hip_clutter_process_dev(blah2hip_clutter_t h, const void *d_x, const void *d_y,
                                 uint32_t n_cpi, uint64_t cpi_stride, void *d_y_out, int32_t *d_ok,
                                 void *stream);
/* The same with the INPUT in format fmt: BLAH2HIP_FMT_C32 (d_x, d_y planes) or BLAH2HIP_FMT_I16 (d_x = the interleaved
 * .rspduo buffer I1 Q1 I2 Q2, d_y ignored: the correlation and FIR kernels read the int16 words directly,
 * RspDuo.cpp:512-526) or BLAH2HIP_FMT_I8 (d_x, d_y planes of int8 pairs, read directly).  A long filter (more than 4081 taps)
 * takes fp32 planes only: BLAH2HIP_ERR_UNSUPPORTED for FMT_I16 and FMT_I8.  The filtered surveillance channel is always written as a complex fp32 plane, CPI c at
 * d_y_out + c * out_stride samples (for FMT_C32 it may alias d_y with out_stride = cpi_stride).  Enqueues only. */
int blah2hip_clutter_process_dev_fmt(blah2hip_clutter_t h, int fmt, const void *d_x, const void *d_y, uint32_t n_cpi,
                                     uint64_t cpi_stride, void *d_y_out, uint64_t out_stride, int32_t *d_ok, void *stream);
/* Several surveillance channels on the same clock against ONE reference (a KrakenSDR; the filter in front of
 * blah2hip_amb_process_multi_dev).  d_y, d_y_out: HOST arrays of n_surv device planes, read at the call; every plane has the
 * layout and stride blah2hip_clutter_process_dev_fmt takes for the same fmt, d_y_out[k] is a complex fp32 plane (FMT_C32: it may
 * alias d_y[k]).  d_y_out = NULL: estimate only, as blah2hip_clutter_estimate_dev_fmt (the taps stay in the handle).
 * What belongs to the reference alone is computed once per CPI instead of once per channel: its autocorrelation r and the
 * spectra every b_k is formed against (shared-reference forms of both correlation kernels; one reduction over 1 + n_surv rows),
 * and the Levinson/Schur recursion on toeplitz(r) (one recursion with n_surv right-hand sides).  The FIR kernel runs once per
 * channel.  r, b_k, the taps and the filtered planes are the BITS of n_surv blah2hip_clutter_process_dev_fmt calls on a handle set
 * to BLAH2HIP_CLUTTER_SOLVE_STEPWISE: the look-ahead solve has no form with several right-hand sides, this entry point always
 * runs the one-workgroup recursion and BLAH2HIP_CLUTTER_INFO_SOLVE_FORM reports _STEPWISE (K per-channel calls keep the
 * look-ahead solve).
 * d_ok: [n_surv][n_cpi] int32, channel-major (NULL: the handle's): the matrix is shared, so the n_surv flags of a CPI are equal;
 * channel k of CPI c is VIRTUAL CPI k * n_cpi + c, as for the maps of blah2hip_amb_process_multi_dev.  Where ok = 0 the taps are
 * zero and NO channel's output is written for that CPI (the single-channel dev calls pass y through there).
 * After this call blah2hip_clutter_read_last and blah2hip_clutter_taps_dev count virtual CPIs: read_last(k * n_cpi + c) returns
 * w_k, r and b_k of CPI c, taps_dev points at [n_surv][n_cpi][n_bins] (a buffer of its own: the pointer differs from the one a
 * single-channel call leaves, which stays valid).  set_timing / get_timing: the BLAH2HIP_CK_* slots, one bracket per stage.
 * fmt: BLAH2HIP_FMT_C32 or BLAH2HIP_FMT_I8; BLAH2HIP_FMT_I16 (one surveillance channel inside the reference's words) is
 * BLAH2HIP_ERR_UNSUPPORTED.  BLAH2HIP_ERR_INVALID: n_surv == 0 or > BLAH2HIP_MAX_SURV, a NULL plane, n_cpi == 0 or > max_batch
 * (max_batch counts CPIs per channel here).  A long filter (more than 4081 taps) runs the per-channel path inside the call,
 * channel after channel: the same result, nothing shared, FMT_C32 only.
 * Enqueues only -- except the first call (and a call with more channels than any before, or the first after a re-planning
 * blah2hip_clutter_set_option), which builds the handle's buffers for n_surv channels: blocking, like the other lazily built state. */
int blah2hip_clutter_process_multi_dev_fmt(blah2hip_clutter_t h, int fmt, const void *d_x, const void *const *d_y, uint32_t n_surv,
                                           uint32_t n_cpi, uint64_t cpi_stride, void *const *d_y_out, uint64_t out_stride,
                                           int32_t *d_ok, void *stream);
/* Execution plan of the filter.  SOLVE_K: indices of the Toeplitz recursion per thread (0 = by
 * size: 1 up to 1024 taps, 2 up to 2048, 4 above; the workgroup has ceil(nBins / K) threads rounded up to a wave). */
#define BLAH2HIP_CLUTTER_OPT_SOLVE_K 1
/* Planner overrides (re-plan and re-allocate the handle's work buffers, blocking; they replace the BLAH2HIP_CLUTTER_FFT_LEN /
 * BLAH2HIP_CLUTTER_CORR environment variables of earlier versions).  FFT_LEN: transform length in {1024, 2048, 4096}, 0 = planner.
 * CORR: BLAH2HIP_CLUTTER_CORR_AUTO / _HALF (two transforms per F/2 samples; needs nBins - 1 <= F/2) / _WINDOW (three per F - nBins + 1). */
#define BLAH2HIP_CLUTTER_OPT_FFT_LEN 2
#define BLAH2HIP_CLUTTER_OPT_CORR 3
#define BLAH2HIP_CLUTTER_CORR_AUTO 0
#define BLAH2HIP_CLUTTER_CORR_HALF 1
#define BLAH2HIP_CLUTTER_CORR_WINDOW 2
/* reported by BLAH2HIP_CLUTTER_INFO_CORR_FORM only, not an option value: a handle with blocks shorter than two filter lengths
 * (n_samples / n_blocks < 2 * n_bins) and no forced form sums r and b lag by lag in fp64 -- such a block's matrix is close to a
 * circulant of the reference's power spectrum, and its condition number (up to 1e6 at n_samples / n_blocks = n_bins) is more
 * than fp32 partial correlations carry */
#define BLAH2HIP_CLUTTER_CORR_DIRECT 3
/* The Toeplitz solve of the normal equations (WienerHopf.cpp:85-122).  SOLVE_FORM: _LOOKAHEAD = blocks of 32 orders on
 * several workgroups per CPI (as many CUs as the launch leaves free; the default), _STEPWISE = the one-workgroup kernel,
 * one barrier per order (SOLVE_K applies to it).  SOLVE_E: indices per lane of the look-ahead form's slices
 * (2, 3, 6 or 12: 96 ... 736 indices per wave; 0 = the smallest whose workgroups each get a CU at the launch's batch). */
#define BLAH2HIP_CLUTTER_OPT_SOLVE_FORM 4
#define BLAH2HIP_CLUTTER_OPT_SOLVE_E 5
/* FIR_CARRY (planner, re-plans like FFT_LEN): 1 (default) = a filter whose history nBins - 1 is just under F/2 (cfg 3: 2047 taps on
 * F = 4096) runs on blocks of exactly F/2 samples and the FIR kernel carries the window overlap in registers; 0 = blocks of
 * F - nBins + 1 samples, every window read whole (tests, A/B timing). */
#define BLAH2HIP_CLUTTER_OPT_FIR_CARRY 6
/* SOLVE_SPIN_LIMIT (tests): polls after which a wait of the look-ahead solve gives up (0 = default, 2^20, about a second).
 * A CPI whose solve gave up is solved again by the one-workgroup kernel enqueued behind it, so a low limit changes the
 * time, not the result. */
#define BLAH2HIP_CLUTTER_OPT_SOLVE_SPIN_LIMIT 7
/* CORR_GRID (tests): workgroups per CPI of the correlation kernels and partials per CPI of the reduction behind them.
 * 0 (default) = the planner's: min(nJobs, two resident generations over the launch's CPIs), nJobs = min(segments, 2 CUs)
 * rounded up to 8.  Any other value must be a multiple of 8 from 8 to that nJobs (the segment walk gives every XCD an
 * eighth of the grid); it holds for every launch of the handle, at any batch, until it is set again or an option that
 * re-plans (FFT_LEN, CORR, FIR_CARRY) returns the handle to 0.  Fewer workgroups than segments make each walk several
 * segments; the sums are the same, their order in fp32 is not.  Not blocking; the next
 * blah2hip_clutter_process_multi_dev_fmt builds its partials again (blocking) where the forced grid needs more of them. */
#define BLAH2HIP_CLUTTER_OPT_CORR_GRID 8
#define BLAH2HIP_CLUTTER_SOLVE_AUTO 0
#define BLAH2HIP_CLUTTER_SOLVE_STEPWISE 1
#define BLAH2HIP_CLUTTER_SOLVE_LOOKAHEAD 2
int blah2hip_clutter_set_option(blah2hip_clutter_t h, int option, int64_t value);
/* What the last process call launched: the solve's form, indices per lane and workgroups per CPI.  The look-ahead
 * form's workgroups wait for each other with BOUNDED waits; a CPI whose wait ran out (workgroups dispatched late on a chip
 * busy with other work) is solved again by the one-workgroup kernel that every look-ahead launch has behind it, gated per
 * CPI, so ok = 0 always and only means "not positive definite" (WienerHopf.cpp:111-115).  SOLVE_FAULT reads
 * (synchronising) the sticky word set when any wait ran out since the handle was created, SOLVE_RETRIES how many CPIs the
 * gated kernel has solved. */
#define BLAH2HIP_CLUTTER_INFO_SOLVE_FORM 1
#define BLAH2HIP_CLUTTER_INFO_SOLVE_E 2
#define BLAH2HIP_CLUTTER_INFO_SOLVE_G 3
#define BLAH2HIP_CLUTTER_INFO_SOLVE_FAULT 4
#define BLAH2HIP_CLUTTER_INFO_SOLVE_RETRIES 5
/* The plan the next process call runs (it follows BLAH2HIP_CLUTTER_OPT_FFT_LEN / _CORR / _FIR_CARRY): CORR_FORM =
 * BLAH2HIP_CLUTTER_CORR_HALF or _WINDOW, FIR_CARRY = 1 where the FIR kernel carries the window overlap in registers,
 * CHUNKS = chunks of 2048 taps of a long filter (more than 4081 taps), 0 for every other. */
#define BLAH2HIP_CLUTTER_INFO_CORR_FORM 6
#define BLAH2HIP_CLUTTER_INFO_FIR_CARRY 7
#define BLAH2HIP_CLUTTER_INFO_CHUNKS 8
/* blocks per CPI (blah2hip_clutter_create_ex), 1 for every other handle */
#define BLAH2HIP_CLUTTER_INFO_BLOCKS 9
/* workgroups per CPI of the handle's last FFT correlation launch (the planner's at that batch, or BLAH2HIP_CLUTTER_OPT_CORR_GRID);
 * 0 before the first, and for the fp64 lag sums of short blocks (BLAH2HIP_CLUTTER_CORR_DIRECT) */
#define BLAH2HIP_CLUTTER_INFO_CORR_GRID 10
int blah2hip_clutter_get_info(blah2hip_clutter_t h, int what, int64_t *value);
/* The filter's Toeplitz solve on its own: n_cpi systems toeplitz(r) w = b given as rb = [n_cpi][2][nBins] complex fp64 (r then b,
 * interleaved re, im; the layout blah2hip_clutter_read_last returns), taps to w ([n_cpi][nBins] complex fp32), ok[c] = 0
 * where the matrix is not positive definite (WienerHopf.cpp:111-115).  Host arrays; synchronises.  For tests and timing of the
 * solve kernels apart from the correlations (set_timing / get_timing: BLAH2HIP_CK_SOLVE). */
int blah2hip_clutter_solve(blah2hip_clutter_t h, const double *rb, uint32_t n_cpi, float *w, int32_t *ok);
/* The same on device-resident arrays; enqueues only. */
int blah2hip_clutter_solve_dev(blah2hip_clutter_t h, const double *d_rb, uint32_t n_cpi, float *d_w, int32_t *d_ok, void *stream);
/* Derived sizes: nBins = delayMax - delayMin taps (WienerHopf.cpp:12), on-chip transform
 * length and samples per overlap-save block. */
int blah2hip_clutter_get_dims(blah2hip_clutter_t h, uint32_t *n_bins, uint32_t *fft_len, uint32_t *seg_len);
/* Copies CPI `cpi` of the last process call's filter to the host (synchronises): the nBins
 * taps w (complex fp32, interleaved), the fp64 correlations the normal equations were built
 * from, r then b (2*nBins complex fp64, interleaved), and the ok flag.  Any output may be NULL.
 * For diagnostics (residual of A w = b) and tests. */
int blah2hip_clutter_read_last(blah2hip_clutter_t h, uint32_t cpi, float *w, double *rb, int *ok);

/* ---- SpectrumAnalyser (SpectrumAnalyser.h:53-62, called blah2.cpp:264) ----
 * decimation = uint32(n/bandwidth), nSpectrum = n/decimation, nfft = nSpectrum*decimation
 * (SpectrumAnalyser.cpp:16-18); spectrum[k] = FFT_nfft(x)[(k*decimation + nfft/2 + 1) mod nfft]
 * (:33-54).  Output: nSpectrum complex fp64 values (re, im interleaved) per CPI.
 * Fails with ERR_INVALID when n < bandwidth (the reference divides by zero), when bandwidth <= 0 or max_batch == 0, and
 * with ERR_UNSUPPORTED when nSpectrum > 2^26 (before anything is allocated). */
int blah2hip_spectrum_create(uint32_t n_samples, double bandwidth, int device, uint32_t max_batch,
                             blah2hip_spectrum_t *out);
int blah2hip_spectrum_destroy(blah2hip_spectrum_t h);
int blah2hip_spectrum_get_dims(blah2hip_spectrum_t h, uint32_t *decimation, uint32_t *n_spectrum, uint64_t *nfft);
/* host: the first nfft of the n samples of the reference channel are used (:33-37) */
int blah2hip_spectrum_process_c64(blah2hip_spectrum_t h, const double *x, uint32_t n, double *spectrum_out);
int blah2hip_spectrum_process_c32(blah2hip_spectrum_t h, const float *x, uint32_t n, double *spectrum_out);
/* dev: d_x in format fmt (C32: complex fp32 plane; I16: the interleaved .rspduo
 * buffer, tuner 1 is used; F16: half pairs; I8: the reference plane of int8 pairs), d_out [n_cpi][nSpectrum] complex fp64.
 * cpi_stride is in SAMPLES in every format, not in bytes or words: CPI i starts 8 (C32: one float pair), 8 (I16: the four
 * int16 words I1 Q1 I2 Q2 of a sample), 4 (F16) or 2 (I8) bytes times i * cpi_stride behind d_x.  It must be >= nfft when
 * n_cpi > 1 and is not used when n_cpi == 1; only the first nfft samples of a CPI are read.  1 <= n_cpi <= max_batch.
 * Refusals (ERR_INVALID: n_cpi, cpi_stride, an fmt other than these four) launch nothing.  Enqueues only. */
int blah2hip_spectrum_process_dev(blah2hip_spectrum_t h, int fmt, const void *d_x, uint32_t n_cpi,
                                  uint64_t cpi_stride, double *d_out, void *stream);

/* ---- the clutter filter's FIR fused into the range correlation (round 6; WienerHopf.cpp:124-160 feeding Ambiguity.cpp:106-149)
 * The filtered surveillance channel never crosses HBM: blah2hip_clutter_estimate_dev_fmt runs the filter's correlations,
 * reduction and Toeplitz solve only (the taps stay in the handle, ok flags as in _process_dev); blah2hip_amb_set_fir hands them
 * to an ambiguity handle, whose next blah2hip_amb_process_dev calls (with the UNFILTERED x, y) filter on the fly inside the range
 * kernel (csrc/kernels.hpp range_fir_kernel).  The result is the two-stage result (same linear operations; fp32 rounding in a
 * different order).  Supported where one 4096-point transform covers it -- the handle's transform length is 4096
 * (BLAH2HIP_OPT_FFT_LEN), n_bins <= 2049, at most 2049 delay bins in one chunk, the filter's first lag equal to the map's and
 * <= 0, symmetric Doppler limits, pulses of at least 2048 - delayMin samples, fp32 or int16 samples (not FMT_F16, and not
 * FMT_I8: the fused kernel has no int8 instantiation, an 8-bit chain runs the two-stage filter) -- else
 * BLAH2HIP_ERR_UNSUPPORTED at the process call.  d_w = NULL switches back to the plain range kernels.  The ambiguity handle keeps
 * the POINTER: the filter handle must outlive its use, and a process call may not ask for more CPIs than the filter handle's max_batch. */
int blah2hip_clutter_estimate_dev_fmt(blah2hip_clutter_t h, int fmt, const void *d_x, const void *d_y, uint32_t n_cpi,
                                      uint64_t cpi_stride, int32_t *d_ok, void *stream);
/* the handle's taps on the device ([max_batch][n_bins] complex fp32; zero where ok = 0), their count and the filter's first lag */
int blah2hip_clutter_taps_dev(blah2hip_clutter_t h, const float **d_w, uint32_t *n_bins, int32_t *delay_min);
int blah2hip_amb_set_fir(blah2hip_amb_t h, const float *d_w, uint32_t n_bins, int32_t clutter_delay_min);
/* BLAH2HIP_OK if the fused kernel covers this handle with such a filter and sample format, else BLAH2HIP_ERR_UNSUPPORTED (the reason
 * in blah2hip_last_error): lets a caller choose between the fused and the two-stage chain before it enqueues anything */
int blah2hip_amb_fir_fusable(blah2hip_amb_t h, int fmt, uint32_t n_bins, int32_t clutter_delay_min);

/* ---- device context for host bindings ------------------------------------
 * What a host-language binding needs of the HIP runtime to keep a CPI resident on the device across the calls
 * of blah2.cpp:264-287 (Spectrum -> WienerHopf -> Ambiguity -> CFAR on the same x, y) without linking it: one
 * stream, pinned staging memory, device buffers and asynchronous copies.  blah2_amd/host/util/DeviceContext
 * builds the per-process sample cache of the drop-in classes on it. */
typedef struct blah2hip_ctx_s *blah2hip_ctx_t;
int blah2hip_ctx_create(int device, blah2hip_ctx_t *out);
int blah2hip_ctx_destroy(blah2hip_ctx_t c);
void *blah2hip_ctx_stream(blah2hip_ctx_t c);                  /* the hipStream_t the dev entry points take */
int blah2hip_ctx_sync(blah2hip_ctx_t c);                      /* waits for everything enqueued on the stream */
int blah2hip_ctx_malloc(blah2hip_ctx_t c, size_t bytes, void **dptr);
int blah2hip_ctx_free(blah2hip_ctx_t c, void *dptr);
int blah2hip_ctx_malloc_host(blah2hip_ctx_t c, size_t bytes, void **hptr); /* pinned */
int blah2hip_ctx_free_host(blah2hip_ctx_t c, void *hptr);
int blah2hip_ctx_h2d(blah2hip_ctx_t c, void *dptr, const void *hptr, size_t bytes); /* enqueues on the stream */
int blah2hip_ctx_d2h(blah2hip_ctx_t c, void *hptr, const void *dptr, size_t bytes); /* enqueues on the stream */
int blah2hip_ctx_d2d(blah2hip_ctx_t c, void *dst, const void *src, size_t bytes);  /* enqueues on the stream */
/* Measurement helper (no reference counterpart): enqueues a kernel that READS `bytes` of device memory at d_src
 * (16-byte aligned) and does nothing else -- the streaming-read rate of the memory system, which bench.py reports
 * beside the copy rate as the ceiling for the range kernel's loads.  d_sink: 4 device bytes, never written, or NULL. */
int blah2hip_stream_read_dev(const void *d_src, size_t bytes, void *d_sink, void *stream);
/* ---- USRP captures --------------------------------------------------------
 * blah2's USRP driver records a two-channel fc32 stream (Usrp.cpp:96-104): per recv() it writes samps_per_buff =
 * B complex<float> of the reference channel x, then B of the surveillance channel y, so sample s of channel c
 * (0 = x, 1 = y) is complex value (s / B) * 2B + c * B + s % B of the file.  B (UHD's get_max_num_samps) is not in
 * the file.  The writer writes all B values even when recv() returned fewer, so such a block ends in stale values;
 * nothing in the file marks it and every block is taken as full.
 * x plane [n_cpi][cpi_stride] and y plane: CPI i sample j = sample (first + i*n_samples + j) of the channel-blocked
 * fc32 buffer d_raw (blocks of `block` complex values, x block then y block).  Enqueue-only on `stream`.
 * Bit-exact copy into BLAH2HIP_FMT_C32 planes; writes n_samples elements per row and nothing beyond.  16-byte accesses
 * when block, first, n_samples and cpi_stride are even and the three pointers 16-byte aligned, 8-byte ones otherwise.
 * BLAH2HIP_ERR_INVALID, with nothing enqueued: NULL pointer, block == 0, n_samples == 0, cpi_stride < n_samples with
 * n_cpi > 1.  n_cpi == 0 enqueues nothing. */
int blah2hip_deblock_c32_dev(const void *d_raw, uint32_t block, uint64_t first, uint32_t n_samples, uint32_t n_cpi,
                             void *d_x, void *d_y, uint64_t cpi_stride, void *stream);
/* device pointers of a handle's internal results of the last blah2hip_amb_process_dev with NULL outputs:
 * map [max_batch][n_doppler][n_delay] complex fp32 and metrics [max_batch][2] doubles */
int blah2hip_amb_result_ptrs(blah2hip_amb_t h, const void **d_map, const double **d_metrics);

/* ---- strong-echo cancellation: least-squares CLEAN on the samples ---------
 * No reference counterpart.  An echo a x[n - d] exp(2 pi i f n / fs) leaves the waveform's own sidelobes in every cell
 * of the map, about n_samples below its peak; the clutter filter removes them at zero Doppler only.  This stage fits
 * the complex amplitudes of a list of ATOMS (d_p, f_p) to the surveillance samples by least squares and subtracts their
 * replicas, so that a second pass of the ambiguity stage sees the floor without them.
 *
 * Definitions (fp64 semantics; blah2_amd.process.clean_replicas / clean_fit / clean_subtract restate them in NumPy).
 * Per CPI, P <= BLAH2HIP_MAX_ATOMS atoms; d_p an integer delay in samples (the units of the map's delay axis; it may be
 * negative), f_p a Doppler in Hz on the map's doppler axis, on a bin or not:
 *   s_p[n] = x[n - d_p] exp(+2 pi i f_p n / fs)   for 0 <= n - d_p < n_samples, 0 elsewhere (nothing wraps)
 *   G[p][q] = sum_n conj(s_p[n]) s_q[n],   b[p] = sum_n conj(s_p[n]) y[n]
 *   G_l = G + loading (tr G / P) I   (the loading rule of blah2hip_amb_mvdr_weights_dev),   G_l a = b
 *   y_out[n] = y[n] - sum_p a_p s_p[n]
 * A noiseless y = s_p peaks in the map cell whose axis values are (d_p, f_p), also on a handle with
 * doppler_middle != 0.  ok = 1 when the Cholesky factor of G_l exists (every pivot finite and above 2^-46 of its
 * loaded diagonal entry: positive beyond the rounding of its own sum) and a is finite; with ok = 0 the amplitudes are 0 and y_out = y bit for bit.  P = 0: ok = 1, y_out = y bit for bit.
 *
 * x is the reference channel in its format, y the surveillance channel as an fp32 plane -- as the clutter filter, a
 * beam former or a C32 capture leaves it: fmt is BLAH2HIP_FMT_C32, _I16X_C32Y or _I8X_C32Y (any other:
 * BLAH2HIP_ERR_UNSUPPORTED).  CPI c of either plane starts c * cpi_stride samples in.  Alignment: fp32 planes 8 bytes,
 * the .rspduo words 4, int8 pairs 2; atoms, amplitudes 8; counts, ok, used 4. */
#define BLAH2HIP_MAX_ATOMS 32
typedef struct blah2hip_clean_s *blah2hip_clean_t;
typedef struct blah2hip_atom {
  int32_t delay;    /* samples */
  int32_t reserved; /* 0 */
  double doppler;   /* Hz */
} blah2hip_atom_t;
/* A canceller for CPIs of n_samples (<= 2^26) samples at fs Hz whose atoms' delays lie in [delay_lo, delay_hi].
 * delay_hi - delay_lo above 4095 is BLAH2HIP_ERR_UNSUPPORTED: the kernels keep a chunk of x plus that halo in LDS.
 * Everything is allocated here (per-workgroup partials, G, b, the amplitudes of max_batch CPIs): the *_dev entry points
 * only enqueue on `stream` and can be captured in a graph.  BLAH2HIP_ERR_INVALID: NULL out, n_samples 0 or above 2^26,
 * fs not finite or not positive, delay_hi < delay_lo, a limit beyond 2^26, a device index out of range. */
int blah2hip_clean_create(uint32_t n_samples, double fs, int32_t delay_lo, int32_t delay_hi, int device, uint32_t max_batch,
                          blah2hip_clean_t *out);
int blah2hip_clean_destroy(blah2hip_clean_t h); /* waits for the device first */
/* BLAH2HIP_CLEAN_OPT_GRAM_GRID: workgroups per CPI of clean_gram_kernel; 0 = the engine's choice (eight a CU over the
 * call).  Whatever is set, a launch has at most one workgroup per chunk of 1024 samples and no more than the handle
 * holds partials for; BLAH2HIP_CLEAN_INFO_GRAM_GRID reads back what the last fit launched, _SUBTRACT_GRID the last
 * subtraction's.  G and b depend on the grid in their last bits only (the fp64 partials are added in a fixed order). */
#define BLAH2HIP_CLEAN_OPT_GRAM_GRID 1
#define BLAH2HIP_CLEAN_INFO_GRAM_GRID 1
#define BLAH2HIP_CLEAN_INFO_SUBTRACT_GRID 2
int blah2hip_clean_set_option(blah2hip_clean_t h, int option, int64_t value);
int blah2hip_clean_get_info(blah2hip_clean_t h, int what, int64_t *value);
/* From final detection lists to atoms; one kernel (clean_atoms_kernel).  d_dets [n_cpi][cap] / d_count [n_cpi] as
 * blah2hip_detect_dev leaves them (a count beyond cap: the first cap records are the list); amb gives the CPI length
 * (dims.cpi) of the Doppler step.  Per CPI the records with snr >= snr_min_db are taken, the strongest first, ties by
 * lower row, then lower col (then lower index), so the result does not depend on the list's order; max_echoes
 * (<= BLAH2HIP_MAX_ATOMS) of them at the most.  Each expands to the cluster (rint(delay) + i, doppler + j 0.5 / cpi),
 * |i| <= side_delay <= 2, |j| <= side_doppler <= 1, written in the order echo, i, j.  A member whose delay is outside
 * [delay_lo, delay_hi] is dropped; an echo whose remaining members do not all fit behind the atoms already written is
 * dropped whole (later, smaller clusters may still fit), as is one with no member left.  d_atoms [n_cpi][cap_atoms],
 * d_atom_count [n_cpi] (never above cap_atoms), d_used [n_cpi][cap_atoms]: the indices into the CPI's list of the
 * detections that gave atoms, in their order, -1 behind them -- what the merge of the two passes' lists needs.
 * BLAH2HIP_ERR_INVALID, nothing enqueued: NULL pointer, n_cpi outside [1, max_batch], cap 0, cap_atoms outside
 * [1, BLAH2HIP_MAX_ATOMS], max_echoes above BLAH2HIP_MAX_ATOMS, a side outside its range, snr_min_db NaN, a buffer off
 * its alignment, an output overlapping an input or another output. */
int blah2hip_clean_atoms_dev(blah2hip_clean_t h, blah2hip_amb_t amb, const blah2hip_det_t *d_dets, uint32_t cap, const uint32_t *d_count,
                             uint32_t n_cpi, double snr_min_db, uint32_t max_echoes, int32_t side_delay, int32_t side_doppler,
                             blah2hip_atom_t *d_atoms, uint32_t cap_atoms, uint32_t *d_atom_count, int32_t *d_used, void *stream);
/* The fit: three kernels.  clean_gram_kernel reads x and y once per CPI: a workgroup walks chunks of 1024 samples,
 * stages the chunk's x window plus the halo delay_hi - delay_lo in LDS, forms the replicas of 128 samples at a time and
 * accumulates the lower triangle of G and b in 4 x 4 register blocks -- fp32 products, fp32 sums over runs of at most 32
 * products, every longer addition in fp64, no floating-point atomics -- and leaves one partial per workgroup;
 * clean_fold_kernel adds the partials in a fixed order -- in index order within 64 contiguous blocks, then the block
 * sums in block order -- (two calls give the same bits; G has exact conjugate symmetry and
 * a real diagonal); clean_solve_kernel factors G_l and solves in fp64.  Replica accuracy: the phase comes from fp64
 * reductions of frac(f n0 / fs) at multiples of 128 samples times a 128-entry table per atom, never from an fp32 product
 * f n: |error| <= 8 2^-24 |x| per sample at every n < n_samples <= 2^26 and |f| <= fs / 2 (clean_kernels.hpp derives
 * 5.8).  d_atom_count[c] beyond cap_atoms: the first cap_atoms atoms are used.  An atom whose delay is outside
 * [delay_lo, delay_hi] or whose Doppler is not finite sets that CPI's ok = 0 (no replica of it is formed).
 * d_amp [n_cpi][cap_atoms] (re, im) doubles, zeros behind the CPI's atoms; d_ok [n_cpi] int32.
 * BLAH2HIP_ERR_INVALID, nothing enqueued: NULL pointer, n_cpi outside [1, max_batch], cap_atoms outside
 * [1, BLAH2HIP_MAX_ATOMS], cpi_stride < n_samples with n_cpi > 1, a buffer off its alignment, loading negative or not
 * finite, an output overlapping an input or the other output. */
int blah2hip_clean_fit_dev(blah2hip_clean_t h, int fmt, const void *d_x, const void *d_y, uint32_t n_cpi, uint64_t cpi_stride,
                           const blah2hip_atom_t *d_atoms, uint32_t cap_atoms, const uint32_t *d_atom_count, double loading,
                           double *d_amp, int32_t *d_ok, void *stream);
/* The subtraction: one kernel (clean_subtract_kernel), the same staging and the same replicas as the fit's.  Per sample
 * y - sum_p a_p s_p is an fp32 chain of fused multiply-adds in atom order, the amplitudes rounded once to fp32:
 * |y_out - (y - S a)| <= about (P + 9) 2^-24 (|y| + sum_p |a_p| |x|) per sample.  16-byte accesses where a CPI's y and
 * output rows both start on 16 bytes, single samples otherwise.  CPIs with ok = 0 or no atoms are copied, or skipped
 * when in place.  d_y_out may be d_y (with out_stride == cpi_stride where n_cpi > 1); the samples of the stride gap are
 * not written.  BLAH2HIP_ERR_INVALID as for the fit, and: out_stride < n_samples with n_cpi > 1, the output overlapping
 * an input other than by that alias. */
int blah2hip_clean_subtract_dev(blah2hip_clean_t h, int fmt, const void *d_x, const void *d_y, uint32_t n_cpi, uint64_t cpi_stride,
                                const blah2hip_atom_t *d_atoms, uint32_t cap_atoms, const uint32_t *d_atom_count, const double *d_amp,
                                const int32_t *d_ok, void *d_y_out, uint64_t out_stride, void *stream);
/* blah2hip_clean_fit_dev followed by blah2hip_clean_subtract_dev; every refusal of either comes before anything is enqueued */
int blah2hip_clean_process_dev(blah2hip_clean_t h, int fmt, const void *d_x, const void *d_y, uint32_t n_cpi, uint64_t cpi_stride,
                               const blah2hip_atom_t *d_atoms, uint32_t cap_atoms, const uint32_t *d_atom_count, double loading,
                               double *d_amp, int32_t *d_ok, void *d_y_out, uint64_t out_stride, void *stream);
/* For tests and diagnosis: waits for the device, then copies CPI `cpi` of the last fit to the host: G [cap][cap] and
 * b [cap] (re, im) doubles with cap = that fit's cap_atoms, the amplitudes [cap] and ok.  Any output may be NULL. */
int blah2hip_clean_read_last(blah2hip_clean_t h, uint32_t cpi, double *G, double *b, double *amp, int32_t *ok);

/* ---- digital down-converter: mix, low-pass and decimate carriers ----------
 * No reference counterpart.  A wideband capture holds several carriers; this stage delivers each of up to
 * BLAH2HIP_MAX_DDC_CARRIERS of them at fs / decim from one pass over the samples, as BLAH2HIP_FMT_C32 planes for the chain
 * behind it.  It works on a two-channel stream u[n] (the reference x and the surveillance y), n the absolute sample index,
 * u[n] = 0 for n < first_sample.  With real taps h[0 .. T-1], the decimation D, the carrier offsets f_c (Hz) and the
 * input rate fs, output m (absolute index; the first is first_sample / D) of carrier c is
 *   v_c[m] = sum_t h[t] u[m D - t] exp(-2 pi i f_c (m D - t) / fs)  =  p_c[m] sum_t g_c[t] u[m D - t]
 *   g_c[t] = fp32(h[t] exp(+2 pi i f_c t / fs)),   p_c[m] = exp(-2 pi i frac(r_c m)),   r_c = f_c D / fs in fp64.
 * The second form is what runs: g_c is made in fp64 at create from exactly reduced arguments and rounded once;
 * each output gets one phasor, r_c m taken with its exact fused residual -- no fp32 product f n exists.  Both
 * channels go through the same taps, so the common group delay of (T - 1) / 2 input samples cancels in the map.
 * blah2_amd.process.ddc restates it in NumPy.  Contract, against that restatement with the read-back g_c:
 *   |v - v_fp64| <= (3 T + 8) 2^-24 sum_t |g_c[t]| |u[m D - t]|   per output
 * (csrc/ddc_kernels.hpp derives it).  int16, int8 and fp32 samples convert exactly.
 * Stream.  A call brings n_rows rows of n_in samples (n_in a multiple of D), consecutive pieces of one stream; the T - 1
 * samples in front of row 0 are the handle's carried history, zeros after create and reset; a call shorter than the
 * history shifts it.  An output's bits depend on its absolute index and the samples under its taps only: the same stream
 * in one call or in any split over rows and calls gives the same bits.  No floating-point atomics. */
#define BLAH2HIP_MAX_DDC_CARRIERS 8
#define BLAH2HIP_MAX_DDC_DECIM 64
#define BLAH2HIP_MAX_DDC_TAPS 1024
typedef struct blah2hip_ddc_s *blah2hip_ddc_t;
/* Host only: a Kaiser-windowed sinc in fp64,
 *   h[t] ~ sinc(2 nu (t - (T-1)/2)) I0(beta sqrt(1 - ((2 t - (T-1)) / (T-1))^2)),   nu = cutoff / (2 decim),
 * sinc(x) = sin(pi x) / (pi x), I0 by its series, normalised to sum h = 1 and symmetric bit for bit (n_taps = 1: h = 1).
 * cutoff is the pass band's edge as a fraction of the output's Nyquist rate.  BLAH2HIP_ERR_INVALID: a NULL table,
 * cutoff outside (0, 1], beta negative or not finite, decim outside [1, BLAH2HIP_MAX_DDC_DECIM], n_taps outside
 * [1, BLAH2HIP_MAX_DDC_TAPS]. */
int blah2hip_ddc_design(uint32_t decim, uint32_t n_taps, double cutoff, double beta, double *h);
/* A down-converter for n_carriers carriers at offset_hz[c] (|f_c| <= fs / 2), calls of at most max_rows (<= 65535) rows of
 * at most max_in (<= 2^30, a multiple of decim) samples.  Everything is allocated here.  BLAH2HIP_ERR_INVALID: a NULL
 * argument, sizes beyond the limits above, fs, a tap or an offset not finite, fs not positive, an offset beyond fs / 2,
 * max_in or max_rows zero or beyond their limits, a device index out of range; the arguments are checked before the
 * device is looked for. */
int blah2hip_ddc_create(double fs, uint32_t decim, const double *h, uint32_t n_taps, const double *offset_hz, uint32_t n_carriers,
                        uint32_t max_in, uint32_t max_rows, int device, blah2hip_ddc_t *out);
int blah2hip_ddc_destroy(blah2hip_ddc_t h); /* waits for the device first */
/* The next call's row 0 starts at absolute sample first_sample (a multiple of decim, else BLAH2HIP_ERR_INVALID); the
 * history is zeroed.  One kernel on `stream`. */
int blah2hip_ddc_reset(blah2hip_ddc_t h, uint64_t first_sample, void *stream);
/* Enqueues ddc_kernel and, behind it, ddc_tail_kernel (the new history and the position, both kept on the device, so a
 * captured graph that is replayed goes on with the stream).  fmt: BLAH2HIP_FMT_C32 (planes d_x, d_y of complex fp32, 8-byte
 * aligned), BLAH2HIP_FMT_I16 (d_x: words I1 Q1 I2 Q2, 8-byte aligned; d_y is not looked at and may be NULL) or
 * BLAH2HIP_FMT_I8 (planes of int8 (I, Q) pairs, 2-byte aligned); any other: BLAH2HIP_ERR_UNSUPPORTED.  Row r of the input
 * starts r * in_stride samples in.  n_out = n_in / decim outputs per row: carrier c, row r of either output plane sits at
 * c * carrier_stride + r * out_stride complex fp32 values, so that every carrier's output is a BLAH2HIP_FMT_C32 batch as it
 * stands; values of the gaps are not written, input values of the gaps not read.
 * A workgroup owns BLAH2HIP_DDC_INFO_TILE consecutive outputs of a row for all carriers and both channels and reads its
 * input window once, into LDS by polyphase (csrc/ddc_kernels.hpp).
 * BLAH2HIP_ERR_INVALID, with nothing enqueued and the stream position unchanged: a NULL pointer, n_in zero, above max_in
 * or no multiple of decim, n_rows zero or above max_rows, in_stride < n_in or out_stride < n_out with n_rows > 1,
 * carrier_stride below a carrier's extent with n_carriers > 1, a buffer off its alignment, an output overlapping an
 * input or the other output. */
int blah2hip_ddc_process_dev(blah2hip_ddc_t h, int fmt, const void *d_x, const void *d_y, uint32_t n_in, uint32_t n_rows, uint64_t in_stride,
                             void *d_out_x, void *d_out_y, uint64_t out_stride, uint64_t carrier_stride, void *stream);
/* the 2 n_taps floats (re, im) of g_c as the kernel multiplies with them, read back from the device */
int blah2hip_ddc_read_taps(blah2hip_ddc_t h, uint32_t carrier, float *g);
/* BLAH2HIP_DDC_INFO_TILE: outputs per workgroup of this handle (a function of decim and n_taps: the window of
 * tile * decim + n_taps - 1 samples fits 80 KB of LDS, two workgroups a CU).  _NEXT_SAMPLE: the absolute index of the
 * next call's first sample, as the calls made through this interface leave it (replays of a captured graph are not
 * counted here; the device's own position follows them). */
#define BLAH2HIP_DDC_INFO_TILE 1
#define BLAH2HIP_DDC_INFO_NEXT_SAMPLE 2
int blah2hip_ddc_get_info(blah2hip_ddc_t h, int what, int64_t *value);

/* ---- multi-carrier integration: carrier maps summed on one velocity axis (no reference counterpart) ----
 * A mast radiates several programmes, and the down-converter above delivers each carrier of a wideband capture.  An echo of
 * bistatic range rate v sits at Doppler -v fc_c / c in carrier c: the same target in ANOTHER ROW of every carrier's map.
 * Summing the power maps of C carriers gives C looks per cell and evens out the programmes' content, once the rows are
 * aligned.  This is one table-driven gather-and-sum over maps that are already on the device.
 *
 * Table.  C <= BLAH2HIP_MAX_CARRIERS carriers with ratio[c] = fc_c / fc_ref; the output axis is the handle's own
 * (blah2hip_amb_get_axes, the reference carrier's).  With doppler[0 .. nD), nD >= 2, D = (doppler[nD-1] - doppler[0]) / (nD - 1),
 * for carrier c and output row j, in fp64, left to right:
 *   u = (ratio[c] * doppler[j] - doppler[0]) / D;   |u - rint(u)| <= 1e-9: u = rint(u)   (ratio 1 is the exact identity)
 * Carrier c COVERS row j when 0 <= u <= nD - 1; otherwise u is clamped to that interval: the edge row stands in, so the cell
 * keeps C looks of noise, and covered[j], the number of carriers that cover row j, tells the caller which rows to distrust.
 *   BLAH2HIP_CARRIER_NEAREST   row = floor(u + 0.5), a_lo = 1, a_hi = 0
 *   BLAH2HIP_CARRIER_LINEAR    row = floor(u), t = u - row, a_hi = fp32(t), a_lo = fp32(1 - t)   (row = nD - 1 implies t = 0)
 * Cell arithmetic.  Input d_map [C][n_cpi][nD][nDelay] complex fp32: what blah2hip_amb_process_dev writes for a batch of
 * C * n_cpi CPIs when the down-converter's carrier_stride is n_cpi * out_stride.  For CPI i, row j, column d, in fp32:
 *   S = 0;  for c = 0 .. C - 1:   p_lo = fmaf(re, re, im * im) of M_c[i][row][d]     (the integrator's form)
 *                                 q = a_lo * p_lo;   a_hi != 0:  q = fmaf(a_hi, p_hi, q), p_hi from row + 1 (else not read)
 *                                 S = fmaf(w_c, q, S)
 *   out[i][j][d] = ( sqrtf(scale * S), 0 ),   scale = fp32(1 / sum_c w_c)
 * -- like the integrator's an ordinary complex map whose |z|^2 is the normalised sum, with Map::set_metrics of the cells as
 * written.  Every term is non-negative: at most 4 roundings up to q, one per carrier in S, one for the scale, halved by
 * the square root, plus its own: the error is below (C + 8) 2^-24 of the cell.  With every ratio 1 either interpolation
 * gives blah2hip_nci_process_dev's bits at window 1 with the same weights.  A NaN cell makes NaN exactly the output cells
 * whose table entries read it.
 * Statistics.  NEAREST keeps a cell exactly Gamma(C) under noise, which is what blah2hip_cfar_alpha(pfa, C, ...) assumes
 * (BLAH2HIP_OPT_CFAR_LOOKS = C); an echo between two rows loses up to 3.9 dB in that carrier.  LINEAR loses less of such an
 * echo, and its cells have lighter tails than Gamma(C) (a convex mix of two cells has a smaller variance), so a detector made
 * for C looks is conservative: its false-alarm rate is below pfa. */
#define BLAH2HIP_MAX_CARRIERS 8
#define BLAH2HIP_CARRIER_NEAREST 0
#define BLAH2HIP_CARRIER_LINEAR 1
/* Host only: the table for this handle's Doppler axis.  row, a_lo, a_hi: [n_carriers][n_doppler]; covered: [n_doppler]; any
 * output pointer may be NULL.  BLAH2HIP_ERR_INVALID: a NULL handle or ratio, n_carriers outside [1, BLAH2HIP_MAX_CARRIERS],
 * a ratio that is not finite or lies outside [0.5, 2], an unknown interpolation, n_doppler < 2. */
int blah2hip_carrier_table(blah2hip_amb_t h, const double *ratio, uint32_t n_carriers, int interp, int32_t *row, float *a_lo,
                           float *a_hi, uint32_t *covered);
/* Builds that table and uploads it into a device buffer the handle owns (allocated at the first call, freed by destroy; the
 * call waits for the device, like blah2hip_amb_set_migration).  n_carriers = 0 clears the table.  BLAH2HIP_ERR_INVALID, with
 * the table that was set left as it was: blah2hip_carrier_table's cases. */
int blah2hip_amb_set_carriers(blah2hip_amb_t h, const double *ratio, uint32_t n_carriers, int interp);
/* The sum for n_cpi CPIs along the table that is set.  d_map: [C][n_cpi][nD][nDelay] (NULL = the handle's internal map behind
 * a process call of C * n_cpi CPIs).  w: HOST array [C] of fp32 weights, read at the call and carried in the launch
 * arguments, or NULL for all 1.  Outputs: d_out_map [n_cpi][nD][nDelay] and d_out_metrics [n_cpi][2].  Enqueues only --
 * carrier_sum_kernel (BLAH2HIP_K_BEAM) and metrics_kernel (BLAH2HIP_K_METRICS), which finishes the metrics in index order
 * (no floating-point atomics) -- with no upload, allocation or synchronisation, and can be captured in a graph.  The
 * workgroups per map (BLAH2HIP_INFO_CARRIER_GRID) depend on the map's geometry alone, never on n_cpi: a map's bits and
 * metrics are the same however the CPIs are cut into calls.  The per-workgroup partials live in the handle's buffers, so
 * calls on one handle must be ordered on the device.
 * BLAH2HIP_ERR_INVALID, with nothing enqueued: a NULL handle or output, no table set, n_cpi == 0 or C * n_cpi above
 * max_batch, a weight that is negative or not finite, weights that add up to 0, a map that is not 8-byte aligned, an output
 * that overlaps the input maps or the other output (the gather cannot run in place).  BLAH2HIP_ERR_UNSUPPORTED: the handle
 * has fewer metrics partials per map than the kernel has workgroups (no geometry the engine plans today). */
int blah2hip_amb_fuse_carriers_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_cpi, const float *w, void *d_out_map,
                                   double *d_out_metrics, void *stream);

/* ---- per-kernel timing (HIP events on the launch stream) ---------------- */
#define BLAH2HIP_K_RANGE 0
#define BLAH2HIP_K_DOPPLER 1
#define BLAH2HIP_K_METRICS 2   /* metrics_kernel: behind the Doppler kernels, the beam former, the integrator, the Doppler taper and walk_sum_kernel */
#define BLAH2HIP_K_CFAR 3     /* cfar1d_kernel, cfar2d_tile_kernel or cfar2d_kernel */
#define BLAH2HIP_K_SAT_ROWS 4 /* 2-D CFAR through the summed-area table (large windows): row prefix sums */
#define BLAH2HIP_K_SAT_COLS 5 /* ... column prefix sums */
#define BLAH2HIP_K_ROTATE 6   /* Doppler-centre shift (asymmetric limits only) */
#define BLAH2HIP_K_BEAM 7     /* beamform_kernel (blah2hip_amb_beamform_dev; its metrics_kernel counts under _METRICS), beam_samples_kernel,
                               * taper_kernel (blah2hip_amb_taper_dev; its metrics_kernel counts under _METRICS too),
                               * carrier_sum_kernel (blah2hip_amb_fuse_carriers_dev; likewise) */
#define BLAH2HIP_K_COV 8      /* array_cov_kernel or sample_cov_kernel + cov_fold_kernel (blah2hip_amb_covariance_dev, _sample_covariance_dev) */
#define BLAH2HIP_K_BEARING 9  /* bearing_kernel (blah2hip_amb_bearing_dev) */
#define BLAH2HIP_K_COUNT 10
/* enable != 0: every dev call brackets each kernel with hipEvents */
int blah2hip_amb_set_timing(blah2hip_amb_t h, int enable);
/* synchronises the recorded events; ms_total[k] = summed duration of kernel k
 * over launches[k] launches since the last reset; then resets */
int blah2hip_amb_get_timing(blah2hip_amb_t h, double *ms_total, uint32_t *launches);
/* the same for the clutter filter's kernels */
#define BLAH2HIP_CK_CORR 0
#define BLAH2HIP_CK_REDUCE 1
#define BLAH2HIP_CK_SOLVE 2
#define BLAH2HIP_CK_FIR 3
#define BLAH2HIP_CK_COUNT 4
int blah2hip_clutter_set_timing(blah2hip_clutter_t h, int enable);
int blah2hip_clutter_get_timing(blah2hip_clutter_t h, double *ms_total, uint32_t *launches);
/* the same for the integrator's kernel, on the integrator: its launches are bracketed there and the ambiguity handle's
 * BLAH2HIP_K_* slots stay as they are (the metrics_kernel behind it counts under the ambiguity handle's BLAH2HIP_K_METRICS) */
#define BLAH2HIP_NK_NCI 0 /* nci_kernel (blah2hip_nci_process_dev) */
#define BLAH2HIP_NK_TRACK_POWER 1 /* track_power_kernel (blah2hip_nci_process_tracks_dev) */
#define BLAH2HIP_NK_TRACK_SUM 2   /* track_sum_kernel (blah2hip_nci_process_tracks_dev) */
#define BLAH2HIP_NK_COUNT 3
int blah2hip_nci_set_timing(blah2hip_nci_t n, int enable);
int blah2hip_nci_get_timing(blah2hip_nci_t n, double *ms_total, uint32_t *launches);
/* the same for the echo canceller's kernels, on its handle */
#define BLAH2HIP_CLK_ATOMS 0    /* clean_atoms_kernel */
#define BLAH2HIP_CLK_GRAM 1     /* clean_gram_kernel */
#define BLAH2HIP_CLK_FOLD 2     /* clean_fold_kernel */
#define BLAH2HIP_CLK_SOLVE 3    /* clean_solve_kernel */
#define BLAH2HIP_CLK_SUBTRACT 4 /* clean_subtract_kernel */
#define BLAH2HIP_CLK_COUNT 5
int blah2hip_clean_set_timing(blah2hip_clean_t h, int enable);
int blah2hip_clean_get_timing(blah2hip_clean_t h, double *ms_total, uint32_t *launches);
/* the same for the down-converter's kernels, on its handle */
#define BLAH2HIP_DK_DDC 0  /* ddc_kernel */
#define BLAH2HIP_DK_TAIL 1 /* ddc_tail_kernel */
#define BLAH2HIP_DK_COUNT 2
int blah2hip_ddc_set_timing(blah2hip_ddc_t h, int enable);
int blah2hip_ddc_get_timing(blah2hip_ddc_t h, double *ms_total, uint32_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* BLAH2HIP_H */

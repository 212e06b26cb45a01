"""The replay chain's config, validated and normalised on the host: :func:`plan_chain` needs no device, no library and no
torch, so every refusal that only the dictionary decides can be had (and tested) anywhere.  :class:`blah2_amd.replay.GpuChain`
builds from the :class:`ChainPlan`; ``replay.main`` plans once before it initialises anything."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from .process import TAPER_COEFFS, ddc_design, rate_bank


def _key(d, name):
    """``d[name]`` of an optional stage: absent, None and False all mean "not configured" and give None."""
    v = (d or {}).get(name)
    return None if v is False else v


def _bank(value, what=""):
    """``QMAX | {max: QMAX, step: S}`` as :func:`blah2_amd.rate_bank` (``what`` names the key inside a larger one)."""
    if isinstance(value, bool):
        raise ValueError(f"{what}QMAX or {{max: QMAX, step: S}}")
    q_max, step = (value.get("max"), value.get("step", 1.0)) if isinstance(value, dict) else (value, 1.0)
    if q_max is None:
        raise ValueError(f"{what}{{max: QMAX, step: S}} needs max")
    return rate_bank(float(q_max), float(step))


def _carrier(fc, offset):
    """A migration or track carrier behind a down-converter at ``offset``: the down-converted carrier's own frequency."""
    fc = float(fc) + offset
    if not math.isfinite(fc) or not fc > 0.0:
        raise ValueError(f"fc = {fc!r} is not a positive, finite frequency")
    return fc


@dataclass(frozen=True)
class ChainPlan:
    """What :func:`plan_chain` returns: one flat record of normalised values, None where a stage is not configured."""
    layout: str
    usrp_block: Optional[int]
    batch: int
    fs_in: int            # the capture's rate and CPI ...
    n_in: int
    fs: int               # ... and the chain's behind the down-converter (the same without one)
    n: int
    fmt_in: int           # the format the filter and the range kernel read
    ddc: Optional[dict]   # {offset, decimation, taps, cutoff, beta} with the defaults filled in (offset: carrier 0's), and "h": the designed low-pass
    taper: Optional[tuple]     # (name, norm)
    migrate_fc: Optional[float]
    rates: Optional[np.ndarray]
    clutter: dict         # {enable, blocks, fused}: fused is the WISH (fir_fusable decides at build)
    integrate: Optional[tuple]  # (W, H)
    tracks: Optional[tuple]     # (fc, bank or None)
    cfar_kind: Optional[str]    # "ca" | "os" | "goca" | "soca", None: detection not enabled
    rank: float
    pfa: Optional[float]  # divided by the rate bank's and the tracks' hypothesis counts (the union bound)
    cmap: Optional[tuple]       # (memory, mode)
    centroid: Optional[int]     # nCentroid
    detect: Optional[str]       # "device" | "host", None without nCentroid
    clean: Optional[dict]       # {snr, echoes, sideDelay, sideDoppler, loading}
    needs_order: bool     # a stage with history from CPI to CPI whatever the batch: one rank only
    cap: Optional[int]    # detection.capacity; None: min(cells of the map, 65536), which the ambiguity handle knows
    carriers: Optional[tuple] = None  # the offsets of several carriers summed on carrier 0's axis; None: one carrier, the chain above
    carrier_interp: str = "nearest"   # capture.ddc.interp: how a carrier's rows are aligned (nearest | linear)
    carrier_fc: Optional[float] = None  # capture.fc, with carriers: the ratios are (fc + offset_c) / (fc + offset_0)


def _plan_ddc(dd, fs_in, n_in, fc=None):
    """(the down-converter's dictionary, the offsets of several carriers or None, the interpolation).  ``offset`` may be a
    list: one entry is the scalar, several are carriers summed on the first one's axis, which need ``fc`` (capture.fc)."""
    # The reader cuts CPIs of n_in samples at fs_in; the chain behind the down-converter runs at fs_in / D on n_in / D.
    try:
        if not isinstance(dd, dict) or dd.get("offset") is None or dd.get("decimation") is None:
            raise ValueError("{offset: HZ, decimation: D, taps: T, cutoff: 0.8, beta: 8} with an offset and a decimation")
        interp = str(dd["interp"]).lower() if dd.get("interp") is not None else "nearest"
        if interp not in _lib.CARRIER_INTERPS:
            raise ValueError(f"interp {interp!r}: 'nearest' or 'linear'")
        carriers, first = None, dd["offset"]
        if isinstance(first, (list, tuple)):
            offs = [float(v) for v in first]
            if not 1 <= len(offs) <= _lib.MAX_CARRIERS:
                raise ValueError(f"{len(offs)} offsets: a list holds 1 .. {_lib.MAX_CARRIERS} carriers")
            carriers, first = tuple(offs) if len(offs) > 1 else None, offs[0]
        if isinstance(dd["decimation"], bool) or int(dd["decimation"]) != dd["decimation"]:
            raise ValueError("decimation is not a whole number")
        D = int(dd["decimation"])
        if not 1 <= D <= _lib.MAX_DDC_DECIM:
            raise ValueError(f"decimation outside [1, {_lib.MAX_DDC_DECIM}]")
        dc = {"offset": float(first), "decimation": D,
              "taps": int(dd["taps"]) if dd.get("taps") is not None else min(16 * D, _lib.MAX_DDC_TAPS),
              "cutoff": float(dd["cutoff"]) if dd.get("cutoff") is not None else 0.8,
              "beta": float(dd["beta"]) if dd.get("beta") is not None else 8.0}
        for off in carriers or (dc["offset"],):
            if not math.isfinite(off) or abs(off) > fs_in / 2:
                raise ValueError("offset not finite or beyond fs / 2")
        if fs_in % D or n_in % D:
            raise ValueError(f"decimation {D} does not divide fs = {fs_in} and the CPI of {n_in} samples")
        if carriers:
            if len(set(carriers)) != len(carriers):
                raise ValueError("two carriers at the same offset")
            if fc is None or isinstance(fc, bool):
                raise ValueError("several carriers need capture.fc, the capture's centre frequency: their Doppler axes scale with fc + offset")
            for off in carriers:
                _carrier(fc, off)  # (refuses an fc + offset that is not positive and finite)
        return dict(dc, h=ddc_design(D, dc["taps"], dc["cutoff"], dc["beta"])), carriers, interp  # (refuses sizes, cutoff and beta outside their ranges)
    except (TypeError, ValueError) as e:
        raise ValueError(f"capture.ddc = {dd!r}: {e}") from None


def _plan_clean(cl_c, device_finisher, integrate, cmap, fp32_plane):
    try:
        if not isinstance(cl_c, dict) or isinstance(cl_c.get("snr"), bool) or not isinstance(cl_c.get("snr"), (int, float)):
            raise ValueError("{snr: dB, echoes: E, sideDelay: 1, sideDoppler: 0, loading: 1e-6} with snr a number of dB")
        cc = {"snr": float(cl_c["snr"]), "echoes": int(cl_c.get("echoes", 4)), "sideDelay": int(cl_c.get("sideDelay", 1)),
              "sideDoppler": int(cl_c.get("sideDoppler", 0)), "loading": float(cl_c.get("loading", 1e-6))}
        if not math.isfinite(cc["snr"]):
            raise ValueError("snr is not finite")
        if not 1 <= cc["echoes"] <= _lib.MAX_ATOMS:
            raise ValueError(f"echoes outside [1, {_lib.MAX_ATOMS}]")
        if not 0 <= cc["sideDelay"] <= 2 or not 0 <= cc["sideDoppler"] <= 1:
            raise ValueError("sideDelay outside [0, 2] or sideDoppler outside [0, 1]")
        if not math.isfinite(cc["loading"]) or cc["loading"] < 0:
            raise ValueError("loading must be finite and not negative")
        if not device_finisher:
            raise ValueError("it reads the final detection lists on the device: detection with nCentroid, and not --detect host")
        if integrate:
            raise ValueError("integrate is configured: the integrator's window would see every CPI twice")
        if cmap:
            raise ValueError("clutterMap is configured: its history would absorb every CPI twice")
        if not fp32_plane:
            raise ValueError("the surveillance channel is not an fp32 plane at that point: it takes a C32 (USRP) "
                             "capture, the down-converter or an enabled clutter filter, whose output is one")
        return cc
    except ValueError as e:
        raise ValueError(f"detection.clean = {cl_c!r}: {e}") from None


def plan_chain(cfg: dict, layout: str = "rspduo", usrp_block: Optional[int] = None, detect: Optional[str] = None,
               batch: int = 1) -> ChainPlan:
    """``cfg`` (the keys :class:`blah2_amd.replay.GpuChain` documents) and the constructor's ``layout``, ``usrp_block``,
    ``detect`` and ``batch`` as a :class:`ChainPlan`, or the ValueError, naming the key, of everything about them that can
    be refused without a handle.  What needs one (a bank or a walk the library refuses, the taper against the Doppler bins,
    the fusable FIR) is refused when the chain is built."""
    if detect not in (None, "device", "host"):
        raise ValueError(f"detect {detect!r}: 'device' or 'host'")
    if layout not in ("rspduo", "usrp", "cs8"):
        raise ValueError(f"layout {layout!r}: 'rspduo', 'usrp' or 'cs8'")
    if layout == "usrp" and (usrp_block is None or int(usrp_block) <= 0):
        raise ValueError("a USRP chain needs the capture's block length (usrp_block > 0)")
    amb_c, det_c, clu_c = cfg["ambiguity"], cfg.get("detection") or {}, cfg.get("clutter") or {}
    fs_in, n_in = int(cfg["fs"]), int(cfg["n_samples"])
    dd = _key(cfg, "ddc")
    ddc, carriers, carrier_interp = _plan_ddc(dd, fs_in, n_in, cfg.get("fc")) if dd is not None else (None, None, "nearest")
    D, offset = (ddc["decimation"], ddc["offset"]) if ddc else (1, 0.0)
    # ambiguity: {window: NAME[:norm]}: the Doppler taper
    win = str(amb_c.get("window") or "none").lower()
    name, _, norm = win.partition(":")
    if norm not in ("", "norm"):
        raise ValueError(f"ambiguity.window {win!r}: NAME or NAME:norm")
    if name not in TAPER_COEFFS:
        raise ValueError(f"ambiguity.window {win!r}: unknown Doppler window {name!r}: one of {', '.join(TAPER_COEFFS)}")
    # ambiguity: {migration: {fc: HZ}}: range-migration compensation for that carrier
    mig, migrate_fc = _key(amb_c, "migration"), None
    if mig is not None:
        if not isinstance(mig, dict) or mig.get("fc") is None:
            raise ValueError("ambiguity.migration needs the carrier frequency: {fc: HZ}")
        try:
            migrate_fc = _carrier(mig["fc"], offset)
        except (TypeError, ValueError) as e:
            raise ValueError(f"ambiguity.migration: {e}") from None
    # ambiguity: {dopplerRate: QMAX | {max: QMAX, step: S}}: the bank -QMAX .. QMAX of Doppler rates
    rate, rates = _key(amb_c, "dopplerRate"), None
    if rate is not None:
        try:
            rates = _bank(rate)
        except (TypeError, ValueError) as e:
            raise ValueError(f"ambiguity.dopplerRate = {rate!r}: {e}") from None
    # integrate: {window: W, hop: H, tracks: {fc: HZ, rate: QMAX | {max: QMAX, step: S}}}; no rate: the bank {0}, the walk only
    int_c, integrate, tracks = cfg.get("integrate"), None, None
    if int_c:
        integrate = (int(int_c["window"]), int(int_c.get("hop") or 1))
        trk = _key(int_c, "tracks")
        if trk is not None:
            try:
                if not isinstance(trk, dict) or trk.get("fc") is None:
                    raise ValueError("needs the carrier frequency: {fc: HZ}")
                rate_t = _key(trk, "rate")
                tracks = (_carrier(trk["fc"], offset), _bank(rate_t, "rate: ") if rate_t is not None else None)
            except (TypeError, ValueError) as e:
                raise ValueError(f"integrate.tracks = {trk!r}: {e}") from None
    enabled = bool(det_c.get("enable", False))
    # detection: {clutterMap: {memory: T, mode: gate | detect}}: every cell against its own history
    cm_c, cmap = _key(det_c, "clutterMap"), None
    if cm_c is not None:
        try:
            if not isinstance(cm_c, dict) or isinstance(cm_c.get("memory"), bool) or not isinstance(cm_c.get("memory"), int):
                raise ValueError("{memory: T, mode: gate | detect} with T a number of CPIs")
            if not 1 <= cm_c["memory"] <= _lib.MAX_CMAP_MEMORY:
                raise ValueError(f"memory outside [1, {_lib.MAX_CMAP_MEMORY}]")
            cmap = (cm_c["memory"], str(cm_c.get("mode", "gate")).lower())
            if cmap[1] not in ("gate", "detect"):
                raise ValueError(f"mode {cmap[1]!r}: 'gate' or 'detect'")
            if not enabled:
                raise ValueError("detection is not enabled")
            if integrate:
                raise ValueError("integrate is configured, and the clutter map's thresholds are made for one look per cell")
        except ValueError as e:
            raise ValueError(f"detection.clutterMap = {cm_c!r}: {e}") from None
    # detection: {cfar: ca | os | goca | soca, rank: 0.75}.  A cell of the rate bank's map is the strongest of K hypotheses, which multiplies
    # the false-alarm rate by at most K: pfa / K (the union bound), and likewise for the hypotheses along the tracks
    kind, pfa, centroid, rank = None, None, None, 0.75
    if enabled:
        kind = str(det_c.get("cfar", "ca")).lower()
        if kind not in ("ca", "os", "goca", "soca"):
            raise ValueError(f"detection.cfar {kind!r}: 'ca', 'os', 'goca' or 'soca'")
        if kind in ("goca", "soca") and (integrate or (carriers and len(carriers) > 1)):
            # greatest-of / smallest-of: the thresholds are made for one look per cell
            raise ValueError(f"detection.cfar {kind!r}: " + ("integrate is configured" if integrate else "several carriers are summed")
                             + ", and the greatest-of / smallest-of thresholds are made for one look per cell")
        pfa = det_c["pfa"] if rates is None else det_c["pfa"] / len(rates)
        if tracks is not None:
            pfa = pfa / (1 if tracks[1] is None else len(tracks[1]))
        centroid = det_c.get("nCentroid")  # blah2.cpp:176-181
        rank = float(det_c.get("rank", 0.75)) if kind == "os" else rank
    where = (detect or "device") if centroid is not None else None
    on = bool(clu_c.get("enable", False))  # clutter: {blocks: K}: taps per block of n / K samples; {fused: false}: two stages
    clutter = {"enable": on, "blocks": int(clu_c.get("blocks", 1)) if on else 1, "fused": on and bool(clu_c.get("fused", True))}
    cl_c, clean = _key(det_c, "clean"), None
    if cl_c is not None:
        clean = _plan_clean(cl_c, where == "device", integrate, cmap, on or layout == "usrp" or ddc is not None)
        clutter["fused"] = False  # the filtered channel has to exist as a plane: the two-stage chain
    if carriers:
        # several carriers: their maps are summed on carrier 0's axis (Ambiguity.fuse_carriers_dev) behind the taper
        C_ = len(carriers)
        looks = C_ * (integrate[0] if integrate else 1)
        for bad, why in ((migrate_fc is not None, "ambiguity.migration is configured: its table is built for one carrier"),
                         (rates is not None, "ambiguity.dopplerRate is configured: its bank is built for one carrier"),
                         (tracks is not None, "integrate.tracks is configured: its tables are built for one carrier"),
                         (cmap is not None, "detection.clutterMap is configured: its thresholds are made for one look per cell"),
                         (clean is not None, "detection.clean is configured: it fits echoes to one carrier's samples"),
                         (where == "host", "--detect host: the fused maps' detections are finished on the device"),
                         (enabled and looks > _lib.MAX_CFAR_LOOKS, f"{looks} looks per cell ({C_} carriers x the integrator's "
                                                                   f"window), above {_lib.MAX_CFAR_LOOKS}")):
            if bad:
                raise ValueError(f"capture.ddc = {dd!r}: {C_} carriers, and {why}")
    fmt_in = _lib.FMT_C32 if ddc else {"rspduo": _lib.FMT_I16, "cs8": _lib.FMT_I8}.get(layout, _lib.FMT_C32)
    return ChainPlan(layout=layout, usrp_block=int(usrp_block) if layout == "usrp" else None, batch=int(batch),
                     fs_in=fs_in, n_in=n_in, fs=fs_in // D, n=n_in // D, fmt_in=fmt_in, ddc=ddc,
                     taper=(name, norm == "norm") if name != "none" or norm else None, migrate_fc=migrate_fc, rates=rates,
                     clutter=clutter, integrate=integrate, tracks=tracks, cfar_kind=kind, rank=rank,
                     pfa=pfa, cmap=cmap, centroid=centroid, detect=where, clean=clean,
                     needs_order=cmap is not None or ddc is not None,
                     cap=int(det_c["capacity"]) if "capacity" in det_c else None,
                     carriers=carriers, carrier_interp=carrier_interp,
                     carrier_fc=float(cfg["fc"]) if carriers else None)

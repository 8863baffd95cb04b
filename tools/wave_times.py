#!/usr/bin/env python
"""Where does each of the 8192 wavefronts of one classify_kernel launch spend its time?  (measurement build -DBNS_WAVE_TIMES; run
with BONSAI_AMD_LIB=<that build>)  Five stamps per wavefront: kernel entry, first claim in hand, first unit finished, last unit
finished, exit.  Prints the percentiles of each as fractions of the kernel's duration, and the share of wave-time (wavefronts x
duration) that lies before a wavefront's first unit has finished and after its last one has.
Three more words per wavefront say what it waited for its claims: the ticks between asking to look at a claim and having it (the
wait in front of the readfirstlane of the atomic's result), summed over its looks, the number of looks, and its longest look.
Printed as "claim_wait": the share of wave-time, the median over the wavefronts of a wavefront's mean look, and the longest look
of the launch, in wall-clock ticks and in microseconds (the wall clock runs at 100 MHz)."""
import ctypes, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench, bonsai_amd

STAMPS = ("entry", "first_claim", "first_unit_done", "last_unit_done", "exit")
WORDS = 8                                  # WAVE_STAMPS of the measurement build: the five stamps, then look ticks, looks, longest look
TICK_US = 0.01
PCTS = (0, 1, 5, 25, 50, 75, 95, 99, 100)

sys.argv = [sys.argv[0], "--no-cpu", "--no-probe", "--steps", "3", "--warmup", "1"] + sys.argv[1:]
# run the bench in-process, then read the stamps of its last launch
orig = bonsai_amd.Context
class Keep(orig):
    def close(self):
        t = np.zeros(WORDS * 8192, dtype=np.uint64)
        self.L.bns_debug_wave_times.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.L.bns_debug_wave_times(self.h, t.ctypes.data)
        t = t.reshape(8192, WORDS).astype(np.int64)
        t = t[t[:, 4] > 0]
        look_ticks, looks, look_max = t[:, 5], t[:, 6], t[:, 7]
        base, end = t[:, 0].min(), t[:, 4].max()
        dur = float(end - base)
        f = (t - base) / dur
        out = {"waves": int(t.shape[0]), "duration_ticks": int(end - base)}
        for i, name in enumerate(STAMPS):
            out[name + "_frac_percentiles"] = {str(p): round(float(np.percentile(f[:, i], p)), 5) for p in PCTS}
        n = float(t.shape[0])
        out["wave_time_share"] = {
            "before_entry": round(float(f[:, 0].sum() / n), 5),
            "entry_to_first_claim": round(float((f[:, 1] - f[:, 0]).sum() / n), 5),
            "first_claim_to_first_unit_done": round(float((f[:, 2] - f[:, 1]).sum() / n), 5),
            "before_first_unit_done": round(float(f[:, 2].sum() / n), 5),
            "after_last_unit_done": round(float((1.0 - f[:, 3]).sum() / n), 5),
            "after_exit": round(float((1.0 - f[:, 4]).sum() / n), 5),
            "resident": round(float((f[:, 4] - f[:, 0]).sum() / n), 5),
        }
        # what a unit takes in the steady state, for scale: (last - first unit done) over the units in between is not known per
        # wavefront, but the first unit's own time against the batch mean is
        out["first_unit_ticks_median"] = float(np.median(t[:, 2] - t[:, 1]))
        asked = looks > 0
        per_look = look_ticks[asked] / looks[asked]
        out["claim_wait"] = {
            "looks": int(looks.sum()),
            "wave_time_share": round(float(look_ticks.sum() / (n * dur)), 5),
            "resident_time_share": round(float(look_ticks.sum() / float((t[:, 4] - t[:, 0]).sum())), 5),
            "per_look_ticks_mean": round(float(look_ticks.sum() / max(1, int(looks.sum()))), 3),
            "per_look_ticks_median_of_wave_means": round(float(np.median(per_look)), 3) if asked.any() else None,
            "per_look_ticks_p95_of_wave_means": round(float(np.percentile(per_look, 95)), 3) if asked.any() else None,
            "per_look_ticks_max": int(look_max.max()),
            "per_look_us_median_of_wave_means": round(float(np.median(per_look)) * TICK_US, 4) if asked.any() else None,
            "per_look_us_max": round(int(look_max.max()) * TICK_US, 3),
        }
        print(json.dumps(out))
        # by XCD (block index mod 8 is the usual round-robin)
        blk = np.arange(8192)[: t.shape[0]] // 4
        for x in range(8):
            sel = (blk % 8) == x
            if sel.any():
                print("xcd-ish %d: median exit %.3f  p95 %.3f" % (x, float(np.median(f[sel, 4])), float(np.percentile(f[sel, 4], 95))))
        super().close()
bonsai_amd.Context = Keep
bench.main()

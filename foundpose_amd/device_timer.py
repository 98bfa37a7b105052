"""Device-event times of a driver's stages (eval_bop19, eval_bop24, eval_coco, gt_info): what their "device_seconds" report."""

from collections import defaultdict
from typing import Dict


class DeviceTimer:
    """timed(kind, fn, ...) calls fn between two HIP events on the current stream; seconds() sums them per kind.  With timing off it only
    calls fn."""

    def __init__(self, timing: bool = True):
        self.timing = timing
        self.events = []

    def timed(self, kind, fn, *a, **kw):
        if not self.timing:
            return fn(*a, **kw)
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a, **kw)
        e1.record()
        self.events.append((kind, e0, e1))
        return out

    def seconds(self) -> Dict[str, float]:
        """Waits for the device; -> the seconds of every kind that was timed."""
        import torch
        torch.cuda.synchronize()
        s = defaultdict(float)
        for kind, e0, e1 in self.events:
            s[kind] += e0.elapsed_time(e1) / 1e3
        return dict(s)

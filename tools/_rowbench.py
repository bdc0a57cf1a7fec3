"""What the bench_* row scripts share: the commit and the device of the header line, the warm-up and timed loops with their wall
line, the profiled pass with its per-kernel lines, and the write-out."""
import os
import subprocess
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 20


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return os.environ.get("VIL_COMMIT", "unknown (not a git checkout)")


def device_name():
    import torch
    return torch.cuda.get_device_name(0)


def timed(fn, calls):
    """WARM calls of fn(), then `calls` timed ones: (what the last warm-up call returned, the wall line)."""
    for _ in range(WARM):
        r = fn()
    ts = []
    for _ in range(calls):
        a = time.perf_counter(); fn(); ts.append(time.perf_counter() - a)
    ts = 1e3 * np.array(ts)
    return r, "wall median %.3f ms, mean %.3f, p90 %.3f, min %.3f" % (np.median(ts), ts.mean(), np.percentile(ts, 90), ts.min())


def profiled(row, fn, calls, unit="call", fmt="    %-18s %4d launches, %8.2f us per launch", idle=True):
    """`calls` more calls with the row's kernel events on: a line per kernel (idle=False: per kernel that ran) and their sum per `unit`."""
    row.profile_enable(True); row.profile_read()
    for _ in range(calls):
        fn()
    prof = row.profile_read()
    out = [fmt % (k, n, 1e3 * ms / max(n, 1)) for k, (n, ms) in prof.items() if n or idle]
    return out + ["    kernels together %8.2f us per %s" % (1e3 * sum(ms for _, ms in prof.values()) / calls, unit)]


def write(lines, out):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "w").write(text)

"""The one place the per-operator bench scripts time and report (scripts/README.md).  Two timing methods, kept apart because the published
figures were taken with them: ``wall_times`` (host clock around a device-synchronised call: what a caller waits for, Python included) and
``event_times`` (a device-event pair around each call: what the stream spends).  Plain functions; the scripts pass ``torch`` in."""
from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np


def wall_times(torch, fn, repeats, warmup):
    """Seconds of ``repeats`` calls, each from a synchronised device to its own synchronise, after ``warmup`` untimed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def wall_time(torch, fn):
    """One such call: a frame of a sequence, where every call is timed and the caller drops the first ones."""
    return wall_times(torch, fn, 1, 0)[0]


def interleaved(torch, calls, repeats, warmup, rounds=3):
    """``{name: [seconds]}``: ``rounds`` rounds over ``calls`` in dictionary order, ``repeats // rounds`` timed calls per entry and round,
    so that a drift of the machine falls on every entry."""
    times = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            times[name] += wall_times(torch, fn, repeats // rounds, warmup)
    return times


def event_times(torch, fns, calls, warmup):
    """(median, p10, p90) in ms of ``calls`` event-timed calls, call q running fns[q % len(fns)]; the warm-up is at least one pass."""
    for q in range(max(warmup, len(fns))):
        fns[q % len(fns)]()
    torch.cuda.synchronize()
    ms = []
    for q in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fns[q % len(fns)]()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return percentiles(ms)


def percentiles(values):
    return float(np.median(values)), float(np.percentile(values, 10)), float(np.percentile(values, 90))


def us_median(seconds):
    return round(1e6 * float(np.median(seconds)), 1)


def us_fields(row, name, seconds):
    """``{name}_us_median`` and ``{name}_us_min`` of a list of seconds, to 0.1 us."""
    row[f"{name}_us_median"], row[f"{name}_us_min"] = us_median(seconds), round(1e6 * float(np.min(seconds)), 1)


def ms_fields(row, name, triple, spread=False, digits=4):
    """``{name}_ms`` of an ``event_times`` triple, with ``spread`` also ``_p10`` / ``_p90``; ``digits=None`` leaves them unrounded."""
    med, p10, p90 = triple if digits is None else (round(v, digits) for v in triple)
    row[name + "_ms"] = med
    if spread:
        row[name + "_ms_p10"], row[name + "_ms_p90"] = p10, p90


def write_rows(rows, out, append, extra=None):
    """Each row, with ``extra`` added, as one flushed JSON line, printed as ``rows`` (a list, or a generator still measuring) hands it
    over, and with ``append`` added to ``out`` at once, so that a run that dies keeps the rows it had; without ``append`` all of them are
    written over ``out`` at the end.  Nothing is written when ``out`` is None.  Returns the rows."""
    done, lines = [], []
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for row in rows:
        done.append({**row, **(extra or {})})
        lines.append(json.dumps(done[-1]) + "\n")
        print(lines[-1], end="", flush=True)
        if out and append:
            with open(out, "a") as f:
                f.write(lines[-1])
    if out and not append:
        with open(out, "w") as f:
            f.writelines(lines)
    return done


def parser(count, count_default, warmup, out=None):
    """The flags every script has: ``--repeats`` / ``--calls`` / ``--frames`` with the script's default, ``--warmup``, ``--out``."""
    ap = argparse.ArgumentParser()
    ap.add_argument(count, type=int, default=count_default)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--out", default=out)
    return ap

"""Host side of per-parameter norm tracking (docs/design/24-norm-tracking.md): what Lightning's `--track_grad_norm` logs as
`grad_2.0_norm/<parameter>` and `grad_2.0_norm_total`, plus weight norms and update-to-weight ratios.  The statistics themselves are
taken on the device (HipAdam.set_norm_tracking, dvq_segment_stats); this module groups the per-parameter dicts of
Trainer.norm_stats() by name prefix, writes `<logdir>/norms.csv`, hands totals to the metrics row and names the parameters whose
gradient turned Inf / NaN.  Standard library only; every aggregation in fp64 (Python floats).

    norms.csv (long format, one line per parameter -- or per prefix group -- per row step):
    step,epoch,opt,name,numel,grad_norm,grad_absmax,grad_nonfinite,weight_norm,update_norm,update_ratio
"""
from __future__ import annotations

import csv
import math
import os

COLUMNS = ("step", "epoch", "opt", "name", "numel", "grad_norm", "grad_absmax", "grad_nonfinite", "weight_norm", "update_norm", "update_ratio")
STATS = ("grad_norm", "grad_absmax", "weight_norm", "update_norm", "update_ratio")       # the scalars of a TensorBoard group
MAX_NAMED = 5                                                                             # parameters named in a non-finite report


def parse_track_grad_norm(value):
    """Lightning's Trainer(track_grad_norm=...): -1 (off, the default), 2 or "inf" -> -1 | 2 | "inf"; anything else raises ValueError"""
    if isinstance(value, str):
        v = value.strip().lower()
        if v == "inf":
            return "inf"
        try:
            value = float(v)
        except ValueError:
            raise ValueError(f"track_grad_norm {value!r}: -1 (off), 2 or 'inf'") from None
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise ValueError(f"track_grad_norm {value!r}: -1 (off), 2 or 'inf'")
    if value == -1:
        return -1
    if value == 2:
        return 2
    if value == math.inf:
        return "inf"
    raise ValueError(f"track_grad_norm {value!r}: -1 (off), 2 or 'inf'")


def total_key(norm_type):
    """Lightning's name of the total: grad_2.0_norm_total / grad_inf_norm_total"""
    return "grad_inf_norm_total" if norm_type == "inf" else "grad_2.0_norm_total"


def _ratio(update_norm, weight_norm):
    if update_norm is None:
        return None
    if weight_norm > 0.0:
        return update_norm / weight_norm
    return 0.0 if update_norm == 0.0 else math.inf


def group_stats(stats, depth=0):
    """{name: entry of HipAdam.norm_stats()} -> {group: {numel, grad_norm, grad_absmax, grad_nonfinite, weight_norm, update_norm,
    update_ratio}} in order of first appearance; a group is the first `depth` dotted components of the name (depth <= 0: the name
    itself).  Sums of squares add, abs-max takes the max, counts add; the ratio is formed from the group's norms."""
    acc = {}
    for name, e in stats.items():
        key = name if depth <= 0 else ".".join(name.split(".")[:depth])
        a = acc.setdefault(key, {"numel": 0, "g2": 0.0, "gmax": 0.0, "bad": 0, "w2": 0.0, "u2": 0.0})
        a["numel"] += int(e["numel"])
        a["g2"] += float(e["grad_norm"]) ** 2
        a["gmax"] = max(a["gmax"], float(e["grad_absmax"]))
        a["bad"] += int(e["grad_nonfinite"])
        a["w2"] += float(e["weight_norm"]) ** 2
        a["u2"] = None if (a["u2"] is None or e.get("update_norm") is None) else a["u2"] + float(e["update_norm"]) ** 2
    out = {}
    for key, a in acc.items():
        wn = math.sqrt(a["w2"])
        un = None if a["u2"] is None else math.sqrt(a["u2"])
        out[key] = {"numel": a["numel"], "grad_norm": math.sqrt(a["g2"]), "grad_absmax": a["gmax"], "grad_nonfinite": a["bad"],
                    "weight_norm": wn, "update_norm": un, "update_ratio": _ratio(un, wn)}
    return out


def totals(stats, norm_type=2):
    """whole-optimizer figures of one stats dict: {"grad_total" (L2 norm, or abs-max with norm_type "inf"), "weight_norm_total",
    "update_ratio_total", "update_ratio_max" (largest per-parameter ratio), "grad_nonfinite"}; the update entries None without them"""
    whole = group_stats({"all." + n: e for n, e in stats.items()}, 1)["all"] if stats else \
        {"grad_norm": 0.0, "grad_absmax": 0.0, "grad_nonfinite": 0, "weight_norm": 0.0, "update_norm": None, "update_ratio": None}
    ratios = [e["update_ratio"] for e in stats.values() if e.get("update_ratio") is not None]
    return {"grad_total": whole["grad_absmax"] if norm_type == "inf" else whole["grad_norm"], "weight_norm_total": whole["weight_norm"],
            "update_ratio_total": whole["update_ratio"], "update_ratio_max": max(ratios) if ratios else None,
            "grad_nonfinite": whole["grad_nonfinite"]}


def metric_row(per_opt_stats, norm_type=2):
    """the keys the metrics logger's `_step` row gains, per optimizer i: grad_2.0_norm_total_opt<i> (or grad_inf_norm_total_opt<i>),
    weight_norm_total_opt<i>, update_ratio_total_opt<i>, update_ratio_max_opt<i>, grad_nonfinite_opt<i>"""
    row = {}
    for i, stats in enumerate(per_opt_stats):
        if stats is None:
            continue
        t = totals(stats, norm_type)
        row[f"{total_key(norm_type)}_opt{i}"] = t["grad_total"]
        row[f"weight_norm_total_opt{i}"] = t["weight_norm_total"]
        if t["update_ratio_total"] is not None:
            row[f"update_ratio_total_opt{i}"] = t["update_ratio_total"]
            row[f"update_ratio_max_opt{i}"] = t["update_ratio_max"]
        row[f"grad_nonfinite_opt{i}"] = t["grad_nonfinite"]
    return row


def nonfinite_report(opt_index, stats, seen_total):
    """one line naming at most MAX_NAMED parameters whose gradient held Inf / NaN elements (running counts, first offending step), or
    None when the optimizer's running total has not grown past `seen_total`; -> (line or None, the new total)"""
    bad = [(n, e) for n, e in stats.items() if e["grad_nonfinite_total"] > 0]
    total = sum(e["grad_nonfinite_total"] for _, e in bad)
    if total <= seen_total:
        return None, seen_total
    bad.sort(key=lambda t: (t[1]["first_bad_step"], -t[1]["grad_nonfinite_total"]))
    named = ", ".join(f"{n} ({e['grad_nonfinite_total']} elements, first at step {e['first_bad_step']})" for n, e in bad[:MAX_NAMED])
    more = f", and {len(bad) - MAX_NAMED} more" if len(bad) > MAX_NAMED else ""
    return f"[norms] opt{opt_index}: non-finite gradient elements in {len(bad)} parameters: {named}{more}", total


class NormsCsv:
    """<logdir>/norms.csv; an existing file -- a resumed run -- is appended to, its header kept"""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        self.path = os.path.join(logdir, "norms.csv")
        if not os.path.exists(self.path) or os.path.getsize(self.path) == 0:
            with open(self.path, "w", newline="") as f:
                csv.writer(f).writerow(COLUMNS)

    @staticmethod
    def _cell(v):
        return "" if v is None else v if isinstance(v, str) else repr(int(v)) if isinstance(v, int) else repr(float(v))

    def write(self, step, epoch, opt_index, grouped):
        with open(self.path, "a", newline="") as f:
            w = csv.writer(f)
            for name, e in grouped.items():
                w.writerow([self._cell(int(step)), self._cell(int(epoch)), self._cell(int(opt_index)), name] +
                           [self._cell(e[k]) for k in COLUMNS[4:]])


class NormTracker:
    """what the Trainer does with the statistics of a row step: norms.csv (with a logdir), TensorBoard scalars norms/<stat>/<group>
    (with a writer), the metrics row's totals, the non-finite report.  Nothing of it is stored in checkpoints."""

    def __init__(self, norm_type=2, depth=0, logdir=None):
        self.norm_type, self.depth = norm_type, max(0, int(depth))
        self.csv = NormsCsv(logdir) if logdir else None
        self._seen_bad = {}
        self.last_row = (None, {})             # (step, metric-row keys) of the last row step

    def row(self, step, epoch, per_opt_stats, tensorboard=None, report=print):
        scalars = {}
        for i, stats in enumerate(per_opt_stats):
            if stats is None:
                continue
            grouped = group_stats(stats, self.depth)
            if self.csv is not None:
                self.csv.write(step, epoch, i, grouped)
            if tensorboard is not None:
                for name, e in grouped.items():
                    for k in STATS:
                        if e[k] is not None and math.isfinite(e[k]):
                            scalars[f"norms/{k}/opt{i}.{name}"] = e[k]
            line, self._seen_bad[i] = nonfinite_report(i, stats, self._seen_bad.get(i, 0))
            if line and report is not None:
                report(line)
        if tensorboard is not None and scalars:
            tensorboard.write(scalars, epoch, step)
        self.last_row = (int(step), metric_row(per_opt_stats, self.norm_type))
        return self.last_row[1]

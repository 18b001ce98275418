"""The files a training run leaves behind, in the formats the reference's analysis reads.

The reference configures baselines' logger on the run directory (run.py:68) and wraps every env in a ``Monitor`` (run.py:81);
its ``plot.py`` / ``viz.ipynb`` / ``baselines.common.plot_util.load_results`` then read

  ``log.txt``            one table per logged update: a dashed line, ``| key | value |`` rows sorted by key, a dashed line.
                         ``plot.py::parse_log`` takes the lines that contain a key and reads ``float(line.split('|')[2].strip())``.
  ``progress.csv``       a header and one row per logged update (``pandas.read_csv``).
  ``0.0.monitor.csv``    ``#{json}`` (``t_start``, ``env_id``), the header ``r,l,t`` and one row per finished episode of agent 0.
  ``early_stop_info.pkl`` / ``ratio_summary.pkl`` / ``eval_against_fix.pkl``   the pickles of alg_ppo.py:427, :466-472 and of the
                         reference's evaluator, which ``plot.py`` loads.

Only these formats are the contract; the code is this project's.  Added here: ``history.json`` (``model.history`` in full) and
``eval_against_fix.json`` (every opponent of the in-training evaluation, train_eval.py).  Plain Python and numpy: no GPU.
"""
import csv
import io
import json
import os
import pickle
import time

import numpy as np

KEY_WIDTH = 30        # log.txt cuts keys and values longer than this to 27 characters plus '...': every key logged here is shorter
MONITOR_FILE = "0.0.monitor.csv"


# ---- log.txt ---------------------------------------------------------------------------------------------------------------
def _cut(s):
    return s[:KEY_WIDTH - 3] + "..." if len(s) > KEY_WIDTH else s


def format_value(v):
    """A number as ``%-8.3g`` (three significant digits, as the reference's log.txt), anything else as ``str``."""
    if isinstance(v, (bool, np.bool_)):
        return str(int(v))
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    if hasattr(v, "__float__"):
        return "%-8.3g" % float(v)
    return str(v)


def format_table(kvs):
    """One update's table: a dashed line, ``| key | value |`` rows sorted by key, a dashed line (with the trailing newline)."""
    rows = [(_cut(str(k)), _cut(format_value(v))) for k, v in sorted(kvs.items())]
    if not rows:
        return ""
    kw, vw = max(len(k) for k, _ in rows), max(len(v) for _, v in rows)
    dashes = "-" * (kw + vw + 7)
    return "\n".join([dashes] + ["| %s%s | %s%s |" % (k, " " * (kw - len(k)), v, " " * (vw - len(v))) for k, v in rows] + [dashes]) + "\n"


# ---- plain values ------------------------------------------------------------------------------------------------------------
def plain_number(v):
    """A logged value as a Python int or float (numpy and torch scalars included): what ``str`` prints round-trips through ``float``."""
    if isinstance(v, (bool, np.bool_)):
        return int(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    return float(v)


def to_jsonable(x):
    """``x`` with numpy / torch scalars and arrays turned into Python numbers and lists, tuples into lists and dict keys into
    strings; None and NaN stay (Python's json writes and reads ``NaN``)."""
    if x is None or isinstance(x, (str, bool, int, float)):
        return x
    if isinstance(x, (np.bool_,)):
        return bool(x)
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    if isinstance(x, np.ndarray):
        return to_jsonable(x.tolist())
    if hasattr(x, "detach") and hasattr(x, "cpu"):                     # torch tensor
        return to_jsonable(x.detach().cpu().numpy())
    if isinstance(x, dict):
        return {str(k): to_jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)) or hasattr(x, "__iter__"):
        return [to_jsonable(v) for v in x]
    raise TypeError("cannot write %r to history.json" % (type(x),))


def _replace(path, data, mode="w"):
    """Write ``data`` to a temporary file next to ``path``, then ``os.replace``: a reader never sees half a file."""
    tmp = path + ".tmp"
    with open(tmp, mode) as f:
        f.write(data)
    os.replace(tmp, path)


def _csv_line(fields):
    buf = io.StringIO()
    csv.writer(buf, lineterminator="\n").writerow(fields)
    return buf.getvalue()


# ---- the run's files ---------------------------------------------------------------------------------------------------------
class RunLog(object):
    """Writes the files of one run into ``log_dir`` (created if missing; files of an earlier run there are overwritten, unless
    ``resume`` -- a :meth:`state` of the interrupted run -- says to continue them).

    ``row(kvs)`` logs one update to ``log.txt`` and ``progress.csv``; ``episodes(epinfos)`` appends a rollout's finished episodes
    to the monitor file; ``history(h)``, ``early_stop_info(l)``, ``ratio_summary(h)`` and ``evaluation(entries)`` rewrite their
    files.  ``header``: extra entries of the monitor file's JSON header (the evaluation opponents' names)."""

    def __init__(self, log_dir, env_id, header=None, resume=None):
        self.dir = str(log_dir)
        os.makedirs(self.dir, exist_ok=True)
        self.monitor_rows = 0
        if resume is not None:
            self._continue(resume)
            return
        self.t_start = time.time()
        self.keys, self.rows = [], []
        for name in ("log.txt", "progress.csv"):
            open(os.path.join(self.dir, name), "w").close()
        head = dict(t_start=self.t_start, env_id=env_id)
        head.update(to_jsonable(header or {}))
        with open(os.path.join(self.dir, MONITOR_FILE), "w") as f:
            f.write("# %s\n" % json.dumps(head))
            f.write("r,l,t\n")

    def state(self):
        """What :meth:`_continue` needs to take the files up where they stand now: the logged rows (exact values), the header of
        progress.csv, the number of monitor rows and ``t_start``.  Small: one dict per logged update."""
        return dict(keys=list(self.keys), rows=[dict(r) for r in self.rows], monitor_rows=int(self.monitor_rows), t_start=self.t_start)

    def _continue(self, st):
        """Continue the files of an interrupted run from ``st`` (a :meth:`state` of it) instead of truncating them: whatever the
        interrupted process wrote after ``st`` was taken is cut off first -- ``log.txt`` and ``progress.csv`` are rewritten from the
        saved rows, byte for byte what they held then, and the monitor file keeps its header and its first ``monitor_rows`` episodes --
        so no update appears twice.  The caller rewrites ``history.json`` and the pickles from the restored history."""
        self.t_start = st["t_start"]
        self.keys, self.rows = list(st["keys"]), [dict(r) for r in st["rows"]]
        self.monitor_rows = int(st["monitor_rows"])
        mon = self.path(MONITOR_FILE)
        if not os.path.exists(mon):
            raise FileNotFoundError("cannot continue the run log: %s is missing" % mon)
        with open(mon) as f:
            lines = f.readlines()
        if len(lines) < 2 + self.monitor_rows:
            raise ValueError("cannot continue the run log: %s holds %d episodes, the saved state %d" % (mon, len(lines) - 2, self.monitor_rows))
        _replace(mon, "".join(lines[:2 + self.monitor_rows]))
        _replace(self.path("log.txt"), "".join(format_table(r) for r in self.rows))
        line = lambda r: _csv_line(["" if k not in r else str(r[k]) for k in self.keys])
        _replace(self.path("progress.csv"), (_csv_line(self.keys) if self.keys else "") + "".join(line(r) for r in self.rows))

    def path(self, name):
        return os.path.join(self.dir, name)

    def row(self, kvs):
        """One logged update.  None values are left out (an empty field of progress.csv).  A key that first appears now goes to
        the end of progress.csv's header and the file is rewritten with the earlier rows padded by empty fields, so the table
        stays rectangular; otherwise the row is appended."""
        kvs = {str(k): plain_number(v) for k, v in kvs.items() if v is not None}
        too_long = [k for k in kvs if len(k) > KEY_WIDTH]
        if too_long:
            raise ValueError("log key %r is longer than %d characters: log.txt would cut it" % (too_long[0], KEY_WIDTH))
        with open(self.path("log.txt"), "a") as f:
            f.write(format_table(kvs))
        new = [k for k in sorted(kvs) if k not in self.keys]
        self.rows.append(kvs)
        line = lambda r: _csv_line(["" if k not in r else str(r[k]) for k in self.keys])
        if new:
            self.keys += new
            _replace(self.path("progress.csv"), _csv_line(self.keys) + "".join(line(r) for r in self.rows))
        else:
            with open(self.path("progress.csv"), "a") as f:
                f.write(line(kvs))

    def episodes(self, epinfos):
        """Append the finished episodes of agent 0 that one rollout harvested (the ``epinfos`` of ``Runner.run``), in harvest order.
        ``t`` is the wall time since ``t_start`` at which the ROLLOUT's harvest is written here (once per update, after its optimiser
        steps), the same for every episode of the update: the device rollout keeps no per-episode clock (the reference's Monitor
        stamps each episode as it ends).  Returns the row count."""
        t = round(time.time() - self.t_start, 6)
        if hasattr(epinfos, "arrays"):
            r, l = epinfos.arrays()
        else:
            r, l = [e["r"] for e in epinfos], [e["l"] for e in epinfos]
        if len(r):
            with open(self.path(MONITOR_FILE), "a") as f:
                f.write("".join("%r,%d,%r\n" % (float(a), int(b), t) for a, b in zip(r, l)))
        self.monitor_rows += len(r)
        return len(r)

    def history(self, history, **extra):
        """``history.json``: ``model.history`` in full (plus ``extra`` entries), rewritten atomically."""
        _replace(self.path("history.json"), json.dumps(to_jsonable(dict(history, **extra))))

    def early_stop_info(self, info):
        """``early_stop_info.pkl`` (alg_ppo.py:427): per update None or [epoch, minibatch] of the KL early stop."""
        _replace(self.path("early_stop_info.pkl"), pickle.dumps(list(info)), "wb")

    def ratio_summary(self, history):
        """``ratio_summary.pkl`` (alg_ppo.py:466-472), nine lists in the reference's slot order.  The reference's list names
        ``off_env_ratio_clip_frac`` in slot 2 (where the plots next to it use ``off_policy_ratio_clip_frac``) and again in slot 4,
        and puts the last update's scalar ``total_clip_frac`` in slot 6; both are kept, so its loaders read what they read there."""
        h = history
        tcf = h["total_ratio_clip_frac"][-1] if h["total_ratio_clip_frac"] else None
        slots = [h["version_gap"], h["off_policy_ratio_mean"], h["off_env_ratio_clip_frac"], h["off_env_ratio_mean"],
                 h["off_env_ratio_clip_frac"], h["total_ratio_mean"], tcf, h["ppo_clip_frac"], h["approxkl"]]
        _replace(self.path("ratio_summary.pkl"), pickle.dumps([list(s) if isinstance(s, list) else s for s in slots]), "wb")

    def evaluation(self, entries):
        """``eval_against_fix.json``: every evaluation entry in full; ``eval_against_fix.pkl``: the reference's layout, a list of
        ``[update, win, draw, lose]`` against the FIRST opponent (what plot.py plots)."""
        _replace(self.path("eval_against_fix.json"), json.dumps(to_jsonable(entries)))
        table = [[int(e["update"])] + [float(e["results"][0][k]) for k in ("win", "draw", "lose")] for e in entries]
        _replace(self.path("eval_against_fix.pkl"), pickle.dumps(table), "wb")


def safemean(xs):
    return np.nan if len(xs) == 0 else float(np.mean(xs))


def last(history, key):
    """The latest entry of a history series, None where the learner keeps no such series or it is empty."""
    s = history.get(key)
    return s[-1] if s else None


def training_row(*, update, nsteps, nbatch, explained_variance, epinfobuf, time_elapsed, loss_names, lossvals, history, league_scores=None,
                 eval_entry=None):
    """The keys of one logged update.  The reference's own (alg_ppo.py:444-458): ``misc/*``, ``eprewmean``, ``epdenserewmean``
    -- computed as the reference computes it: its line 449 averages ``epinfo['r']`` again, so it EQUALS ``eprewmean`` --
    ``eplenmean`` and ``loss/<name>``.  Added: throughput and phase times, the opponent's version and its gap to the learner
    (update - 1 - version, the ``version_gap`` of the 'random' mode), the three importance-ratio means and clip fractions,
    ``useful_ratio``, the env's fault counters, the learner's estimated win rate per league member (``league/<k>/win``) and, for
    an update that was evaluated, ``eval/<k>/win|draw|lose`` against evaluation opponent k.  Series a learner does not keep (the
    A2C learner has no ratios) and None values are left out."""
    r = [e["r"] for e in epinfobuf]
    kv = {"misc/serial_timesteps": update * nsteps, "misc/nupdates": update, "misc/total_timesteps": update * nbatch,
          "misc/explained_variance": float(explained_variance), "eprewmean": safemean(r), "epdenserewmean": safemean(r),
          "eplenmean": safemean([e["l"] for e in epinfobuf]), "misc/time_elapsed": time_elapsed}
    for name, v in zip(loss_names, lossvals):
        kv["loss/" + name] = float(v)
    for k in ("fps", "rollout_s", "update_s", "useful_ratio", "off_policy_ratio_mean", "off_env_ratio_mean", "total_ratio_mean",
              "off_policy_ratio_clip_frac", "off_env_ratio_clip_frac", "total_ratio_clip_frac"):
        kv[k] = last(history, k)
    opp = last(history, "opponent_versions")
    if opp:
        kv["opponent_version"], kv["version_gap"] = int(opp[0]), update - 1 - int(opp[0])
    for k in ("diverged", "dropped_contacts", "rollout_aborts"):
        kv["env/" + k] = last(history, "env_" + k)
    for k, row in enumerate(league_scores or ()):          # rows of (episodes, learner wins, losses, draws), policy_zoo.league_scores
        kv["league/%d/win" % k] = row[1] / row[0] if row[0] else np.nan
    if eval_entry is not None:
        for k, res in enumerate(eval_entry["results"]):
            for name in ("win", "draw", "lose"):
                kv["eval/%d/%s" % (k, name)] = res[name]
    return kv

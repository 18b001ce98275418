#!/usr/bin/env python3
"""Pictures of one or more training runs, drawn from the files ``run.py`` leaves in a run directory (robosumo_selfplay_amd/runlog.py).
The panel types are those of the reference's plot.py, read from the same files:

    python plot_run.py --runs results/RoboSumo-Ant-vs-Ant-v0-0 --type train_reward --out reward.png
    python plot_run.py --runs results/RoboSumo-Ant-vs-Ant-v0-{0,1,2} --type eval_against_fix --out eval.png
    python plot_run.py --runs results/RoboSumo-Ant-vs-Ant-v0-0 --type losses --out losses.png

  train_reward       ``eprewmean`` over ``misc/total_timesteps`` (progress.csv)
  eval_against_fix   win rate against the first evaluation opponent and the score 2000 win - 1000 draw - 2000 lose over the
                     update (eval_against_fix.pkl, rows ``[update, win, draw, lose]``); the other opponents' win rates, dashed,
                     where eval_against_fix.json holds them
  losses             every ``loss/*`` column, ``misc/explained_variance``, ``eplenmean`` and ``eprewmean`` (progress.csv)

Runs given together are taken as seeds of one experiment: where their x axes agree they are averaged into one curve (the
reference's plots do the same), otherwise every run is drawn on its own.
"""
import argparse
import json
import os
import pickle
import sys

import numpy as np


def load_progress(run):
    import pandas as pd
    return pd.read_csv(os.path.join(run, "progress.csv"))


def load_eval(run):
    """(updates, [win, draw, lose] columns) of the first opponent, sorted by update, and the other opponents' win rates by name."""
    with open(os.path.join(run, "eval_against_fix.pkl"), "rb") as f:
        rows = sorted(pickle.load(f), key=lambda x: x[0])
    others = {}
    path = os.path.join(run, "eval_against_fix.json")
    if os.path.exists(path):
        with open(path) as f:
            entries = sorted(json.load(f), key=lambda e: e["update"])
        for e in entries:
            for k, r in enumerate(e["results"][1:], 1):
                others.setdefault("%d: %s" % (k, os.path.basename(r["opponent"])), []).append((e["update"], r["win"]))
    return np.array([r[0] for r in rows], float), np.array([r[1:4] for r in rows], float).reshape(len(rows), 3), others


def curves(xs, ys, labels):
    """Seeds averaged where every run has the same x axis; otherwise one curve per run.  Returns [(x, y, label)]."""
    same = all(len(x) == len(xs[0]) and np.array_equal(x, xs[0]) for x in xs)
    if len(xs) > 1 and same:
        return [(xs[0], np.nanmean(np.stack(ys), axis=0), "mean of %d runs" % len(xs))]
    return list(zip(xs, ys, labels))


def draw(ax, xs, ys, labels, title, **kw):
    for x, y, label in curves(xs, ys, labels):
        ax.plot(x, y, label=label, **kw)
    ax.set_title(title, fontsize=9)


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", nargs="+", required=True, help="run directories (run.py --log_path/<env>-<suffix>)")
    ap.add_argument("--type", required=True, choices=["train_reward", "eval_against_fix", "losses"])
    ap.add_argument("--out", required=True, help="the picture to write: FILE.png (the format follows the extension: .svg, .pdf)")
    args = ap.parse_args(argv)
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    labels = [os.path.basename(os.path.normpath(r)) for r in args.runs]
    if args.type == "train_reward":
        prog = [load_progress(r) for r in args.runs]
        fig, ax = plt.subplots(figsize=(8, 4.5))
        draw(ax, [p["misc/total_timesteps"].to_numpy(float) for p in prog], [p["eprewmean"].to_numpy(float) for p in prog], labels, "eprewmean")
        ax.set_xlabel("timesteps")
        ax.legend(fontsize=7)
    elif args.type == "eval_against_fix":
        ev = [load_eval(r) for r in args.runs]
        fig, (ax1, ax2) = plt.subplots(1, 2, figsize=(11, 4.5))
        xs = [e[0] for e in ev]
        draw(ax1, xs, [e[1][:, 0] for e in ev], labels, "win rate against the first opponent")
        for e, label in zip(ev, labels):
            for name, pts in sorted(e[2].items()):
                ax1.plot([p[0] for p in pts], [p[1] for p in pts], "--", linewidth=0.8, label="%s [%s]" % (label, name))
        draw(ax2, xs, [2000.0 * e[1][:, 0] - 1000.0 * e[1][:, 1] - 2000.0 * e[1][:, 2] for e in ev], labels,
             "2000 win - 1000 draw - 2000 lose")
        ax1.set_ylim(-0.02, 1.02)
        for ax in (ax1, ax2):
            ax.set_xlabel("update")
        ax1.legend(fontsize=6)
    else:
        prog = [load_progress(r) for r in args.runs]
        cols = [c for c in prog[0].columns if c.startswith("loss/")] + ["misc/explained_variance", "eplenmean", "eprewmean"]
        cols = [c for c in cols if all(c in p.columns for p in prog)]
        n = max(1, len(cols))
        ncol = min(4, n)
        nrow = -(-n // ncol)
        fig, axes = plt.subplots(nrow, ncol, figsize=(4 * ncol, 3 * nrow), squeeze=False)
        for ax, c in zip(axes.ravel(), cols):
            draw(ax, [p["misc/nupdates"].to_numpy(float) for p in prog], [p[c].to_numpy(float) for p in prog], labels, c)
        for ax in axes.ravel()[len(cols):]:
            ax.axis("off")
        axes.ravel()[0].legend(fontsize=6)
    fig.tight_layout()
    fig.savefig(args.out, dpi=100)
    plt.close(fig)
    return args.out


if __name__ == "__main__":
    main(sys.argv[1:])

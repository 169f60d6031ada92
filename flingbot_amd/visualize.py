"""python -m flingbot_amd.visualize DIR [--replay replay.npz ...]

The reference's `python visualize.py <log>/replay_buffer.hdf5` for a report directory written by
`python -m flingbot_amd.evaluate ... --report DIR` (or --lane-report / --probe-report DIR: a probed map's row shows its lattice
regret, Spearman, chosen rank and concordant pairs): prints the summary of the replay files that are named
(report.summarize: collect_stats' scalars and the episode lengths per difficulty) and (re)writes DIR/index.html from
DIR/actions.jsonl (report.write_report).  Needs no GPU: the strips were composed during the run."""
import argparse


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("directory", metavar="DIR", help="a report directory (evaluate's --report, --lane-report or --probe-report DIR)")
    ap.add_argument("--replay", nargs="+", default=[], metavar="REPLAY.npz", help="files written by evaluate's --dump")
    return ap


def main(argv=None):
    from .report import summarize, write_report

    a = build_parser().parse_args(argv)
    if a.replay:
        summarize(a.replay)
    print(write_report(a.directory))


if __name__ == "__main__":
    from flingbot_amd.visualize import main as _package_main

    _package_main()

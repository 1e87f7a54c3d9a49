"""What tools/gen_vae_golden.py and tools/gen_score_golden.py share: the repository on sys.path, the fixture directory, the command line."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def open_reference(families, only):
    """[--reference DIR] [--family NAME ...] [--only ...] -> (the chosen families, args.only, the reference's models, its utils)"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=G.REF)
    ap.add_argument("--family", nargs="+", choices=list(families), default=list(families))
    ap.add_argument("--only", choices=only)
    a = ap.parse_args()
    G.REF = a.reference
    net, rutils = G.import_reference()
    torch.set_num_threads(8)      # (reduction order, and with it the last bits of a fixture, depends on the thread count)
    return a.family, a.only, net, rutils


def widened(make, sd):
    """make() in float64, loaded with the fp32 numbers `sd`: the float64 runs start from what the fp32 runs start from"""
    m = make().double()
    m.load_state_dict({k: v.double() for k, v in sd.items()})
    return m

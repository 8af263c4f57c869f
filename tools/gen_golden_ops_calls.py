#!/usr/bin/env python
"""Records tests/golden/ops_calls.json: the C-ABI calls every op of tripled_amd.ops makes when it is driven forward and backward
on CPU tensors against a stand-in library -- the driver is tests/ops_calls_util.py, the one tests/test_ops_calls_cpu.py runs.
Needs neither the built library nor a GPU.

  python tools/gen_golden_ops_calls.py [--out tests/golden/ops_calls.json]

The file pins the marshalling of ops.py / native.py, so it is regenerated ONLY with a deliberate change of the C ABI or of what
an op launches -- never to make a refactor of the Python side pass: read the diff of the JSON (one case per line) as part of
that change's review.
"""
import argparse
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import ops_calls_util  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=ops_calls_util.golden_path(ROOT))
    args = ap.parse_args()
    with pytest.MonkeyPatch.context() as mp:
        text = ops_calls_util.dumps(ops_calls_util.record(mp.setattr))
    with open(args.out, "w") as f:
        f.write(text)
    print("%s: %d cases, %d bytes" % (args.out, text.count("\n") - 2, len(text)))


if __name__ == "__main__":
    main()

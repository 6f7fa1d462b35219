"""The single-process exchange trace, recorded — TEST INFRASTRUCTURE.

mvg_debug_trace_exchange lists the calls one process driving G devices issues for the exchange:
the communicator splits, then one multiply's collectives and exact mode's combine. This writes
what the built library records at 96 x 96 for every algorithm, G in {1, 2, 3, 4, 6, 8} (all of
which split 96 x 96 under all three algorithms; the grid is 2 x 3 at G = 6 and 2 x 4 at G = 8),
tree and exact, to tests/golden/exchange_traces.json: {"<alg>/G<g>/<tree|exact>": [calls]}, a
call being the fields of mvg_xcall in declaration order. tests/test_capi_host.py compares the
library's trace with it call for call, so a change to the engine that alters which buffers a
rank owns, which exchange it picks or in which order it issues the calls shows on a CPU.

Regenerate only when the schedule is meant to change: python tests/golden/make_exchange_traces.py
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

R = C = 96
ALGS = ("rowwise", "colwise", "blockwise")
DEVICES = (1, 2, 3, 4, 6, 8)


def cases():
    for alg in ALGS:
        for g in DEVICES:
            for exact in (False, True):
                yield f"{alg}/G{g}/{'exact' if exact else 'tree'}", alg, g, exact


def main() -> None:
    from matvec_mpi_multiplier_amd import _lib
    from matvec_mpi_multiplier_amd import multiplier as mm

    fields = [name for name, _ in _lib.XCall._fields_]
    traces = {key: [[c[f] for f in fields] for c in mm.trace_exchange(alg, R, C, g, exact)]
              for key, alg, g, exact in cases()}
    path = os.path.join(HERE, "exchange_traces.json")
    with open(path, "w") as f:
        f.write('{"generator": "tests/golden/make_exchange_traces.py", "R": %d, "C": %d,\n' % (R, C))
        f.write(' "fields": %s,\n "traces": {\n' % json.dumps(fields))
        f.write(",\n".join('  "%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in traces.items()))
        f.write("\n }}\n")
    print(f"wrote {len(traces)} traces, {sum(map(len, traces.values()))} calls, to {path}")


if __name__ == "__main__":
    main()

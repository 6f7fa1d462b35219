"""The single-process exchange trace, recorded — TEST INFRASTRUCTURE.

mvg_debug_trace_exchange lists the calls one process driving G devices issues for the exchange:
the communicator splits, then one multiply's collectives and exact mode's combine. This writes
what the built library records at 96 x 96 for every algorithm, G in {1, 2, 3, 4, 6, 8} (all of
which split 96 x 96 under all three algorithms; the grid is 2 x 3 at G = 6 and 2 x 4 at G = 8),
tree and exact, to tests/golden/exchange_traces.json: {"<alg>/G<g>/<tree|exact>": [calls]}, a
call being the fields of mvg_xcall in declaration order. tests/test_capi_host.py compares the
library's trace with it call for call, so a change to the engine that alters which buffers a
rank owns, which exchange it picks or in which order it issues the calls shows on a CPU.

The same cases for a block of NV = 3 vectors (mvg_debug_trace_exchange_multi: one
multiply_multi's exchange) go to tests/golden/exchange_traces_multi.json, the same format plus
"nv".

Regenerate only when the schedule is meant to change: python tests/golden/make_exchange_traces.py
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

R = C = 96
NV = 3
ALGS = ("rowwise", "colwise", "blockwise")
DEVICES = (1, 2, 3, 4, 6, 8)


def cases():
    for alg in ALGS:
        for g in DEVICES:
            for exact in (False, True):
                yield f"{alg}/G{g}/{'exact' if exact else 'tree'}", alg, g, exact


def trace_multi(alg, R, C, ndev, exact, nv):
    """mvg_debug_trace_exchange_multi's calls as dicts in issue order."""
    from matvec_mpi_multiplier_amd import _lib

    cap = (16 * ndev + 16) * (nv + 1)
    calls = (_lib.XCall * cap)()
    n = ctypes.c_int()
    _lib.check(_lib.lib.mvg_debug_trace_exchange_multi(_lib.ALG_BY_NAME[alg], R, C, ndev, int(exact), nv, calls, cap,
                                                       ctypes.byref(n)), "mvg_debug_trace_exchange_multi")
    return [calls[i].as_dict() for i in range(n.value)]


def write(name, head, fields, traces):
    path = os.path.join(HERE, name)
    with open(path, "w") as f:
        f.write('{"generator": "tests/golden/make_exchange_traces.py", %s,\n' % head)
        f.write(' "fields": %s,\n "traces": {\n' % json.dumps(fields))
        f.write(",\n".join('  "%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in traces.items()))
        f.write("\n }}\n")
    print(f"wrote {len(traces)} traces, {sum(map(len, traces.values()))} calls, to {path}")


def main() -> None:
    from matvec_mpi_multiplier_amd import _lib
    from matvec_mpi_multiplier_amd import multiplier as mm

    fields = [name for name, _ in _lib.XCall._fields_]
    write("exchange_traces.json", '"R": %d, "C": %d' % (R, C), fields,
          {key: [[c[f] for f in fields] for c in mm.trace_exchange(alg, R, C, g, exact)]
           for key, alg, g, exact in cases()})
    write("exchange_traces_multi.json", '"R": %d, "C": %d, "nv": %d' % (R, C, NV), fields,
          {key: [[c[f] for f in fields] for c in trace_multi(alg, R, C, g, exact, NV)]
           for key, alg, g, exact in cases()})


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates tests/golden/verify_verdicts.json on a GPU: what every verifier of csrc/verify.hip answers to the proofs and
mutations of tests/verify_verdicts.py -- status, *accept, the smi_last_error sentence, consumed, n_pv and a checksum of the
polynomial values.  The fixture pins the verifiers' observable behaviour across changes to their code: it is made ONCE, at
the commit whose behaviour is to be kept, and not regenerated when verify.hip is reorganised.

    python tests/golden/make_verify_verdicts.py        # rewrites verify_verdicts.json (needs the GPU)

Sentences no well-formed request reaches are listed, with the reason, in verify_verdicts.UNREACHABLE."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import stark_rs_amd as s
    import air_compose as ac
    import verify_verdicts as vv
    from oracle import oracle as o
    o.build()
    o.lib()
    engines = {p: s.Engine(p, g, 0) for p, g in ac.PRIMES}
    t0 = time.time()
    table = vv.run_all(engines, o)
    dt = time.time() - t0
    seen = {row[4] for rows in table.values() for row in rows}
    missing = [x for x in vv.SENTENCES if x not in seen and x not in vv.UNREACHABLE]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "verify_verdicts.json")
    vv.dump(table, out)
    print("wrote", out, os.path.getsize(out), "bytes;", sum(map(len, table.values())), "verdicts in %.1f s" % dt)
    for k, rows in table.items():
        print("%5d  %s" % (len(rows), k))
    print("sentences never seen:", missing)
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())

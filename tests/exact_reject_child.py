"""Run as a child process by tests/test_exact_words_cpu.py: every ill-sorted
query of tests/exactcases.py through ms_solve and ms_session_solve.  A query
the blaster reads out of bounds on kills this process, not pytest.  Prints one
JSON line per row as it goes (what each call answered), then ``DONE n``."""
import json
import sys

import exactcases as X
from mythril_amd.smt import exact
from mythril_amd.smt.expr import symbol_factory as sf


def answer(solver, conj, session):
    try:
        st, _ = solver._check(conj, (), 20000, session, solver.max_conflicts)
        return st
    except exact.Unsupported:
        return "Unsupported"


def main():
    rows = [(rule, label, conj) for rule, label, conj in X.ill_sorted_rows()]
    rows += [("kernel-2 program", label, conj) for label, conj in X.ill_sorted_programs()]
    out = []
    x = sf.BitVecSym("x", 256)
    for rule, label, conj in rows:
        stateless = answer(exact.ExactSolver(session=False), conj, False)
        s = exact.ExactSolver()
        # the session holds a well-sorted query before the ill-sorted one, and
        # decides one after it (on a new session: the rejected one is closed)
        before = s.check([(x + 1 == x).raw])[0]
        in_session = answer(s, conj, True)
        closed = s._session is None
        after = s.check([(x * 3 == 7).raw])
        ok_after = after[0] == "sat" and (after[1]["x"] * 3) % (1 << 256) == 7
        s.close()
        fresh = exact.ExactSolver()
        ok_fresh = fresh.check([(x + 1 == x).raw])[0] == "unsat" and fresh.check([(x * 3 == 7).raw])[0] == "sat"
        fresh.close()
        out.append({"rule": rule, "label": label, "python": X.sort_error(conj), "ms_solve": stateless,
                    "ms_session_solve": in_session, "session_closed": closed, "before": before,
                    "decides_after": ok_after, "fresh_decides": ok_fresh})
        print(json.dumps(out[-1]), flush=True)
    print("DONE", len(out))


if __name__ == "__main__":
    sys.exit(main())

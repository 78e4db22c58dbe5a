"""Child process of tests/test_linear_exact_gpu.py: started with SELFOCC_LINEAR_B3=0, runs the reduced exact list on the f32-MFMA
kernels and prints one JSON line per case.  Exit status 0 = every case ran (the parent asserts on the lines)."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import linear_cases as lc  # noqa: E402


def main():
    from selfocc_amd.linear import linear_fwd, linear_wgrad
    env = os.environ.get("SELFOCC_LINEAR_B3")
    for (T, N, K) in lc.CHILD_FWD:
        for fam in lc.FAMILIES:
            c = lc.fwd_case(fam, T, N, K)
            x, w, b = c['x'].cuda(), c['w'].cuda(), c['bias'].cuda()
            y = linear_fwd(x, w, b)
            diff = (y.double().cpu() - (c['want'] + c['bias'].double())).abs().max().item()
            print(json.dumps(dict(op="fwd", family=fam, shape=[T, N, K], b3_env=env, exact=diff == 0.0, max_diff=diff,
                                  repeat_identical=bool(torch.equal(linear_fwd(x, w, b), y)))), flush=True)
    for (T, N, K) in lc.CHILD_WGRAD:
        for fam in ('A', 'C', 'D'):
            c = lc.wgrad_case(fam, T, N, K, False)
            dy, x = c['dy'].cuda(), c['x'].cuda()
            dw, db = linear_wgrad(dy, x)
            diff = max((dw.double().cpu() - c['want_w']).abs().max().item(), (db.double().cpu() - c['want_b']).abs().max().item())
            dw2, db2 = linear_wgrad(dy, x)
            print(json.dumps(dict(op="wgrad", family=fam, shape=[T, N, K], b3_env=env, exact=diff == 0.0, max_diff=diff,
                                  repeat_identical=bool(torch.equal(dw, dw2) and torch.equal(db, db2)))), flush=True)


if __name__ == "__main__":
    main()

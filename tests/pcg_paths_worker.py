"""Worker of test_gpu_pcg.py::test_pcg_under_process_wide_switches: OBHIP_HM3 and OBHIP_HESSMULT_FUSED are
read once per process, so the checks of test_gpu_pcg.py under either run in a process of their own.
Usage: pcg_paths_worker.py <OBHIP_HM3 | OBHIP_HESSMULT_FUSED> (the variable itself set to 0 by the parent);
prints "pcg paths ok <variable>" at the end."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conftest  # noqa: E402,F401  (puts the oracle on the path)
import test_gpu_pcg as T  # noqa: E402

var = sys.argv[1]
assert os.environ.get(var) == "0", var
for name in ("small", "star300"):
    q = T.check_shape(name)
    if var == "OBHIP_HM3":
        # k_hm2 where k_star<OP_HESS> would run (p = 2500): still enqueued ahead, still batched
        batched = True
    else:
        # no k_hm2 / k_star: k_hm_tl or two kernels with k_cg_q, nothing speculative
        batched = False
    T.check_problem(q, "%s %s=0" % (name, var), q.case["ladder"], batched=batched)
print("pcg paths ok " + var, flush=True)

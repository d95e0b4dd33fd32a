"""us per timestep of an unarmed resident run (no recorder) on the reference's 128^2 and 1024^2 data sets: 4000-step calls,
median of 5 after a warm-up.
python tools/resident_unarmed.py [checkout]     the built checkout to measure (default: this one; tools/probes_ab.sh
alternates this one and the parent commit's)"""
import os
import statistics
import sys
import time

root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(root, "tests"))
import conftest  # noqa: E402

lbm = conftest.load_package()
steps = 4000
out = []
for name in ("128x128", "1024x1024"):
    p, ob = conftest.dataset(name)
    p.max_iters = 7 * steps
    with lbm.Engine(p, ob) as eng:
        assert eng.info()["resident_steps"] > 0
        t = []
        for i in range(6):
            eng.sync()
            t0 = time.perf_counter()
            eng.run(steps)
            eng.sync()
            if i:
                t.append((time.perf_counter() - t0) / steps * 1e6)
        out.append(f"{name} {statistics.median(t):.3f} us/step")
print("resident unarmed: " + "  ".join(out), flush=True)

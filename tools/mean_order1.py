"""us per timestep of a resident run with the order-1 mean fields armed (Engine.set_mean, which the parent commit of the
second moments has too), next to the same engine unarmed: 128^2, 256^2 and 1024^2 data sets, 4000-step calls, median of 5
after a warm-up, the recorder re-armed outside the timed region before every call.
python tools/mean_order1.py [checkout]     the built checkout to measure (default: this one; tools/mean_ab.sh alternates
this one and the parent commit's)"""
import os
import statistics
import sys
import time

root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(root, "tests"))
import conftest  # noqa: E402

lbm = conftest.load_package()
steps = 4000
for name in ("128x128", "256x256", "1024x1024"):
    p, ob = conftest.dataset(name)
    p.max_iters = 30 * steps
    with lbm.Engine(p, ob) as eng:
        assert eng.info()["resident_steps"] > 0
        out = []
        for label, every in (("unarmed", 0), ("mean /100", 100), ("mean /10", 10), ("mean /1", 1)):
            t = []
            for i in range(6):
                eng.set_mean(every)
                eng.sync()
                t0 = time.perf_counter()
                eng.run(steps)
                eng.sync()
                if i:
                    t.append((time.perf_counter() - t0) / steps * 1e6)
            out.append(f"{label} {statistics.median(t):.3f}")
        print(f"{name:>10}: us/step  " + "  ".join(out), flush=True)

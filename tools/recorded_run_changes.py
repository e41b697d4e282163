import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "compressor-mpc_amd"))
import bench  # noqa: E402

t = time.time()
r = bench.recorded_run_changes(0, int(sys.argv[1]))
print(json.dumps(r), time.time() - t)

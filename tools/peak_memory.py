"""Device memory in use at the peak of a command: `python tools/peak_memory.py -- python bench.py --steps 20 --warmup 5` runs the command
as a child process and polls hipMemGetInfo of device 0 from this one, five times a second; prints one JSON line when the child ends.
The figure includes this process's own HIP context (a few hundred MB), the same for every build compared."""
import json
import subprocess
import sys
import time

import torch

cmd = sys.argv[sys.argv.index("--") + 1:]
free0, total = torch.cuda.mem_get_info(0)
child = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
low = free0
while child.poll() is None:
    low = min(low, torch.cuda.mem_get_info(0)[0])
    time.sleep(0.2)
print(json.dumps({"command": " ".join(cmd), "rc": child.returncode, "total_bytes": total, "in_use_before": total - free0, "in_use_at_peak": total - low}))

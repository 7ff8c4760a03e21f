"""Seconds of masp_hip_circuit_load and device memory taken across the call (hipMemGetInfo before / after), per circuit, one context,
Spend then Output then Convert; one JSON line.  MASP_HIP_LIBRARY selects the build (MEASUREMENTS.md "Quotient in evaluation form")."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import masp_amd
from masp_amd import host as H, synthetic
ctx = masp_amd.Context(0)
out = {"library": os.environ.get("MASP_HIP_LIBRARY", "branch")}
for slot, kind in enumerate(("spend", "output", "convert")):
    cs = H.circuit(kind)[0]
    params = ctx.generate_parameters(cs, synthetic.toxic_waste(1 + slot))
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    ctx.load_circuit(slot, params, cs)
    dt = time.perf_counter() - t0
    free1 = torch.cuda.mem_get_info()[0]
    form = ctx.circuit_quotient_form(slot) if hasattr(ctx._L, "masp_hip_circuit_quotient_form") else None
    out[kind] = {"load_s": round(dt, 3), "device_bytes": free0 - free1, "form": form}
ctx.close()
print(json.dumps(out))

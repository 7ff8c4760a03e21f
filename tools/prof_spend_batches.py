"""Three full Spend batches of 256 proofs through masp_hip_prove_batch and nothing else: the program of a `rocprofv3 --kernel-trace --stats`
run of its own.  MASP_HIP_LIBRARY selects the build (MEASUREMENTS.md "Quotient in evaluation form")."""
import os, random, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import masp_amd
from masp_amd import host as H, synthetic, workload as W
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
ctx = masp_amd.Context(0)
cs = H.circuit("spend")[0]
params = ctx.generate_parameters(cs, synthetic.toxic_waste(1))
ctx.load_circuit(0, params, cs)
insts = W.instances("spend", 256, first_seed=1000)
rng = random.Random(5)
for _ in range(3):
    ctx.prove_batch([(0, i, a, rng.randrange(R), rng.randrange(R)) for i, a in insts])
ctx.close()
print("3 batches of 256 Spend proofs")

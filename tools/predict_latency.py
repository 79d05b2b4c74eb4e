"""End-to-end latency of NNetWrapper.predict_batch for one position (host call + uploads + forward + downloads);
--leaves-per-step K: for K positions, the batch a one-game search with leaves_per_step = K hands the network."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from othellozero_amd.NNet import NNetWrapper
K = int(sys.argv[sys.argv.index("--leaves-per-step") + 1]) if "--leaves-per-step" in sys.argv else 1
for prec in ("f16x2", "f32"):
    net = NNetWrapper((8, 8), num_channels_1=512, max_batch=K, seed=0, precision=prec)
    own = np.array([0x0000000810000000] * K, dtype=np.uint64); opp = np.array([0x0000001008000000] * K, dtype=np.uint64)
    for _ in range(20): net.predict_batch(own, opp)
    t0 = time.perf_counter()
    N = 500
    for _ in range(N): net.predict_batch(own, opp)
    dt = (time.perf_counter() - t0) / N
    print(f"{prec}: {dt * 1e6:.1f} us per predict_batch({K})   (GPU forward alone: {net.time_forward(K, 50) * 1e3:.1f} us)", flush=True)

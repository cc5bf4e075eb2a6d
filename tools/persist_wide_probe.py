"""Persistent reverse sweep (k_adj_persist) at ensemble widths: device time of the reverse sweep per stage and per member-stage, 128x128
quads with contact at the records checkpoint level, for several members per launch and for a wide ensemble cut into consecutive launches.
    python tools/persist_wide_probe.py [STEPS] [ARM ...]      ARM = MEMBERS[:VAR=VAL,VAR=VAL...]
Default arms: 1, 2 and 3 members (one launch each), 32 members on the persistent reverse (one stream group, forced with
DFX_PERSIST_CHUNKS=16 DFX_STREAMS=1), 32 members on stage launches (DFX_PERSIST=0) and 32 members as the engine chooses (two stream groups)."""
import os
import sys
import time

import numpy as np

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
from common import Case  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
DEFAULT = ["1", "2", "3", "32:DFX_PERSIST_CHUNKS=16,DFX_STREAMS=1", "32:DFX_PERSIST=0,DFX_STREAMS=1", "32:DFX_STREAMS=2"]
arms = []
for a in (sys.argv[2:] or DEFAULT):
    b, _, env = a.partition(":")
    arms.append((int(b), dict(kv.split("=") for kv in env.split(",")) if env else {}))
T = 5
ts = np.linspace(0.0, 1e-3, T)
spi = max(1, steps // (T - 1))
n_steps = spi * (T - 1)
for B, env in arms:
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = Case("quads", 128, True, True, seed=100, lib=None, cutoff_deg=-10.0, batch=B)
        cp = c.cp._replace(constraint_params=dict(amplitude=7.5, loading_rate=1000.0, input_delay=1e-5))
        nb = c.geo.n_blocks
        target = np.array([nb // 2 + 1, nb // 2 + 2], dtype=np.int32)
        y0 = np.zeros((2, nb, 3))
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            c.solver(y0, ts, [cp] * B if B > 1 else cp, keep_trajectory=True, steps_per_interval=spi, want_fields=False)
            st = dict(c.solver.stats)
            c.solver.kinetic_energy_value_and_raw(target)
            sa = dict(c.solver.adjoint_stats)
            wall = time.perf_counter() - t0
            if best is None or sa["kernel_ms"] < best[1]["kernel_ms"]:
                best = (st, sa, wall)
        st, sa, wall = best
        n_stage = n_steps * 6
        us = 1e3 * sa["kernel_ms"] / n_stage
        print(f"quads 128 x {B} members, {n_steps} steps, {env or 'defaults'}: reverse {us:.2f} us/stage = {us / B:.3f} us per member-stage "
              f"(build {sa.get('tile_kernels')}, {sa.get('launches')} launches, {sa.get('streams')} streams, level records={sa.get('checkpoint_records')}); "
              f"forward {1e3 * st['kernel_ms'] / n_stage:.2f} us/stage (build {st['tile_kernels']}); wall {wall * 1e3:.1f} ms", flush=True)
        del c
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

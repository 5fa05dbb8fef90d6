"""Timing of the `fxs average` step for dimensions = 2 on the device (xframe_amd/fxs/average.py: average_reconstructions_2d): R
synthetic reconstructions at N shells x M -- perturbed copies of one asymmetric density, every other one point-inverted -- centred,
normalised, un-inverted against the best one, averaged, with PRTF, pseudo FSC and FQCB.  Also times the same flow through the numpy
restatement of the reference's run_2d (tests/average2d_reference.py on the transforms of oracle/polar2d.py) on this host.
Writes a report: wall times, time and calls per operator (every operator call ends with a stream synchronisation, so its wall time
is its kernels' time plus the launch and synchronisation overhead), the launch count and the share spent in transfers.
usage: bench_average2d.py [N M n_batch [output file]]   (default 128 64 8 profiles/average2d_timing.txt; R = 8 and 100)"""
import os
import sys
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import torch                                          # noqa: E402
import average2d_reference as AR                      # noqa: E402
from oracle import polar2d as OP                      # noqa: E402
from xframe_amd.fxs import average as AV              # noqa: E402
from xframe_amd.fxs.polar2d import Engine2D           # noqa: E402

N, M, B = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (128, 64, 8)
OUT = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, 'profiles', 'average2d_timing.txt')
MAX_Q = 2.0
LAUNCHES = {'t_fourier_transform': 3, 't_harmonic': 1}            # per chunk of n_batch; every other operator is one launch per call
OPS = ('t_fourier_transform', 't_harmonic', 't_grid_stats', 't_inversion_metric', 't_phase_ramp', 't_combine', 't_curves', 't_fqcb',
       't_deg2_from_table')
lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)


def problem(e, R, seed=11):
    rng = np.random.default_rng(seed)
    r, p = np.meshgrid(e.rs, e.phis, indexing='ij')
    x, y, rmax = r * np.cos(p), r * np.sin(p), r.max()

    def blob(cx, cy, w):
        return np.exp(-((x - cx * rmax) ** 2 + (y - cy * rmax) ** 2) / (w * rmax) ** 2)
    base = (blob(0.15, -0.1, 0.2) + 0.6 * blob(-0.25, 0.2, 0.12)) * (1 + 0.3j) - 0.05 * blob(0, 0, 0.45)
    rho = []
    for i in range(R):
        c = 0.3 * rng.normal(size=(3, 2))
        rho.append(base * (1.0 + 0.02 * i) + sum(0.1 * (1 + 0.5j * k) * blob(c[k, 0], c[k, 1], 0.15) for k in range(3)))
    rho = np.stack(rho)
    F = e.t_fourier_transform(rho)
    inv = e.t_fourier_transform(F.conj(), True)
    recs = [[inv[i], F[i].conj()] if i % 2 else [rho[i], F[i]] for i in range(R)]
    errors = 1.0 + rng.random(R)
    errors[R // 2] = 0.5
    pms = [[(rng.normal(size=N) + 1j * rng.normal(size=N)) for _ in range(M + 1)]]
    return recs, errors, pms


class Meter:
    """wall time and calls per Engine2D operator, uploads (Alignment2D.to_device) and downloads (Tensor.cpu)"""

    def __init__(self, e):
        self.e, self.t, self.n, self.launches = e, defaultdict(float), defaultdict(int), 0
        self.saved = {}

    def wrap(self, obj, name, key, count=None):
        fn = getattr(obj, name)
        self.saved[(obj, name)] = fn
        meter = self

        def timed(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            meter.t[key] += time.perf_counter() - t0
            meter.n[key] += 1
            if count is not None:
                meter.launches += count(*a, **k)
            return out
        setattr(obj, name, timed)

    def __enter__(self):
        B_ = self.e.B
        for op in OPS:
            per = LAUNCHES.get(op)
            self.wrap(self.e, op, op, (lambda X, *a, _p=per, **k: _p * -(-int(X.shape[0]) // B_)) if per else (lambda *a, **k: 1))
        self.wrap(AV.Alignment2D, 'to_device', 'upload')
        cpu = torch.Tensor.cpu
        self.saved[(torch.Tensor, 'cpu')] = cpu
        meter = self

        def timed_cpu(x, *a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = cpu(x, *a, **k)
            meter.t['download'] += time.perf_counter() - t0
            meter.n['download'] += 1
            return out
        torch.Tensor.cpu = timed_cpu
        return self

    def __exit__(self, *exc):
        for (obj, name), fn in self.saved.items():
            if obj is self.e:
                delattr(obj, name)
            else:
                setattr(obj, name, fn)


def wall(fn, reps=3):
    best = None
    for rep in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rep == 0:
            first = dt
        else:
            best = dt if best is None else min(best, dt)
    return first, best, out


opt = {'center_reconstructions': True, 'normalize_reconstructions': {'use': True, 'mode': 'max'}, 'selection': {'n_reconstructions': 1000},
       'resolution_metrics': {'PRTF': True, 'pseudo_FSC': True, 'FQCB': True}}
e = Engine2D(N, M, MAX_Q, n_batch=B)
fp = OP.PolarFourierPair(N, M, MAX_Q)
fl = AR.Flow2D(fp.rs, fp.qs, fp.n_phi, fp.ft, fp.ift, OP.harmonic_forward)
say(f'average_reconstructions_2d at {N} shells x M = {M} (rows of {2 * M + 1}), engine n_batch = {B}, metrics PRTF + pseudo_FSC + FQCB')
say(f'device: {torch.cuda.get_device_name(0)}')
say('transfers: "upload" is the conversion of the input arrays to device tensors, "download" every Tensor.cpu() of the result.  Copies made')
say('inside an operator -- its few scalars per grid coming back, a host array argument staged by the library -- count as that')
say('operator\'s time, so the transfer share is a lower bound for host-array input.')
for R in (8, 100):
    recs, errors, pms = problem(e, R)
    dv = e.torch_device()
    recs_dev = [[torch.from_numpy(a).to(dv), torch.from_numpy(b).to(dv)] for a, b in recs]
    say()
    say(f'---- {R} reconstructions')
    f, b, got = wall(lambda: AV.average_reconstructions_2d(e, recs, errors, opt, pms))
    say(f'host arrays in, result on the host:                 first call {1e3 * f:8.1f} ms, best of the next 2 {1e3 * b:8.1f} ms')
    f, b, _ = wall(lambda: AV.average_reconstructions_2d(e, recs_dev, errors, dict(opt, keep_on_device=True, FQCB_bl_arrays=False), pms))
    say(f'device tensors in, aligned pairs stay, no B_n arrays: first call {1e3 * f:8.1f} ms, best of the next 2 {1e3 * b:8.1f} ms')
    t0 = time.perf_counter()
    ref = AR.run_2d_ref(fl, recs, errors, opt, pms)
    t_np = time.perf_counter() - t0
    say(f'numpy restatement of run_2d on this host (one run):  {1e3 * t_np:8.1f} ms')
    err = np.linalg.norm(got['average']['real_density'] - ref['average']['real_density']) / np.linalg.norm(ref['average']['real_density'])
    say(f'averaged density, device against the restatement: relative L2 {err:.2e}; point inverted {sum(got["point_inverted"])} of {R - 1}')
    with Meter(e) as m:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        AV.average_reconstructions_2d(e, recs, errors, opt, pms)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    say(f'one metered run (host arrays in, result on the host; metering adds synchronisations): {1e3 * total:.1f} ms, {m.launches} kernel launches')
    say(f'  {"operator":<22}{"calls":>7}{"ms":>10}{"share":>8}')
    for key in OPS + ('upload', 'download'):
        if m.n[key]:
            say(f'  {key:<22}{m.n[key]:>7}{1e3 * m.t[key]:>10.2f}{100 * m.t[key] / total:>7.1f}%')
    # (downloads inside operators -- their few scalars per grid -- are counted with the operator)
    rest = total - sum(m.t.values())
    say(f'  {"host logic, torch glue":<22}{"":>7}{1e3 * rest:>10.2f}{100 * rest / total:>7.1f}%')
    say(f'  transfers (upload + download): {100 * (m.t["upload"] + m.t["download"]) / total:.1f}% of the run')
e.close()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')

"""Test-side float64 reference of ``powerflow.solved_case`` (include/gns_powerflow.h, "The solved case"), independent of the product:
the forward from ``ac_contingency_reference.branch_flows`` / ``line_admittances`` and ``nr_reference.ybus`` / ``roles`` / ``specified``
in numpy, ties decided by ``ac_contingency_reference.extreme``; the gradients from torch float64 autograd on the CPU over a torch
restatement of the same formulas (the injections there as the sum of the flows that leave a bus plus its shunt, which is the same
quantity by another route).  Everything is for ONE grid: raw ``[N,6]``, ``[E,7]``, ``[Gn,7]`` arrays, ``v``, ``theta`` ``[N]``."""
from collections import namedtuple

import numpy as np
import torch

import ac_contingency_reference as aref
import nr_reference as nr

FLOAT_OUT = ('p_from', 'q_from', 'p_to', 'q_to', 'p_inj', 'q_inj', 'mismatch', 'gen_p', 'gen_q', 'slack_p', 'worst_loading', 'v_min',
             'v_max')
INDEX_OUT = ('worst_line', 'v_min_bus', 'v_max_bus')
# the differentiable outputs (mismatch is not), and the columns the contract gives a gradient
DIFF_OUT = ('p_from', 'q_from', 'p_to', 'q_to', 'p_inj', 'q_inj', 'gen_p', 'gen_q', 'slack_p', 'worst_loading', 'v_min', 'v_max')
DIFF_COLS = {'buses': [2, 3, 4, 5], 'lines': [2, 3, 4, 5, 6], 'generators': [6]}

Case = namedtuple('Case', FLOAT_OUT + INDEX_OUT + ('gaps', 'from_end'))


def _units(gen, slack):
    """(0-based bus of every unit, units per bus as a dict, the units listed on the slack in listing order)."""
    gb = np.asarray(gen, dtype=np.float64)[:, 0].astype(int) - 1
    count = {}
    for b in gb.tolist():
        count[b] = count.get(b, 0) + 1
    return gb, count, [u for u in range(gb.size) if gb[u] == slack]


def forward(buses, lines, generators, slack_bus, v, theta, rating=None):
    """The ``Case`` of one grid at (v, theta).  ``gaps``: the distance of each summary to its runner-up at another index
    (``worst_loading``, ``v_min``, ``v_max``); ``from_end``: whether the from end of ``worst_line`` attains the loading."""
    bus, ln, gen = (np.asarray(a, dtype=np.float64) for a in (buses, lines, generators))
    v, theta = np.asarray(v, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    pf, qf, pt, qt = aref.branch_flows(ln, v, theta)
    V = v * np.exp(1j * theta)
    S = V * np.conj(nr.ybus(bus, ln) @ V)
    p_inj, q_inj = S.real.copy(), S.imag.copy()
    slack, pv, pq = nr.roles(bus, gen, slack_bus)
    mis = S - nr.specified(bus, gen)
    terms = np.r_[mis[np.r_[pv, pq]].real, mis[pq].imag]
    mismatch = float(np.max(np.abs(terms), initial=0.0)) if np.all(np.isfinite(terms)) else float('nan')
    gb, count, on_slack = _units(gen, slack)
    gen_q = np.array([(q_inj[b] + bus[b, 3]) / count[b] for b in gb.tolist()], dtype=np.float64).reshape(gb.size)
    gen_p = gen[:, 6].copy()
    ps = p_inj[slack] + bus[slack, 2]
    if on_slack:
        gen_p[on_slack[0]] = ps - sum(gen[u, 6] for u in on_slack[1:])
    slack_p = ps - sum(gen[u, 6] for u in on_slack)
    sf, st = np.hypot(pf, qf), np.hypot(pt, qt)
    load = np.maximum(sf, st) if rating is None else np.maximum(sf, st) / np.asarray(rating, dtype=np.float64)
    wl, wi, wgap = aref.extreme(load)
    lo, lo_i, lo_gap = aref.extreme(v, largest=False)
    hi, hi_i, hi_gap = aref.extreme(v)
    return Case(pf, qf, pt, qt, p_inj, q_inj, mismatch, gen_p, gen_q, float(slack_p), wl, lo, hi, wi, lo_i, hi_i,
                dict(worst_loading=wgap, v_min=lo_gap, v_max=hi_gap), bool(sf[wi] >= st[wi]))


def torch_outputs(bus, ln, gen, v, theta, slack_bus, rating, at):
    """The differentiable outputs as torch float64 tensors of torch float64 inputs (a dict by name).  ``at``: the indices the summaries
    are taken at, frozen: ``worst_line``, ``from_end``, ``v_min_bus``, ``v_max_bus`` (a ``Case`` has them)."""
    f = torch.as_tensor(ln[:, 0].detach().numpy().astype(int) - 1)
    t = torch.as_tensor(ln[:, 1].detach().numpy().astype(int) - 1)
    ys = 1.0 / torch.complex(ln[:, 2], ln[:, 3])
    tap = torch.polar(ln[:, 5], ln[:, 6])
    ytt = ys + 1j * ln[:, 4] / 2
    yff = ytt / (tap * tap.conj())
    yft = -ys / tap.conj()
    ytf = -ys / tap
    V = torch.polar(v, theta)
    sf = V[f] * (yff * V[f] + yft * V[t]).conj()
    st = V[t] * (ytf * V[f] + ytt * V[t]).conj()
    n = bus.shape[0]
    S = torch.zeros(n, dtype=torch.complex128).index_add(0, f, sf).index_add(0, t, st) + v * v * torch.complex(bus[:, 4], bus[:, 5]).conj()
    slack = int(slack_bus) - 1
    gb, count, on_slack = _units(gen.detach().numpy(), slack)
    gbt = torch.as_tensor(gb)
    per_unit = torch.as_tensor([1.0 / count[b] for b in gb.tolist()], dtype=torch.float64).reshape(gb.size)
    gen_q = (S.imag[gbt] + bus[gbt, 3]) * per_unit
    ps = S.real[slack] + bus[slack, 2]
    gen_p = gen[:, 6]
    if on_slack:
        first = torch.zeros(gb.size, dtype=torch.bool)
        first[on_slack[0]] = True
        others = sum((gen[u, 6] for u in on_slack[1:]), torch.zeros((), dtype=torch.float64))
        gen_p = torch.where(first, ps - others, gen_p)
    slack_p = ps - sum((gen[u, 6] for u in on_slack), torch.zeros((), dtype=torch.float64))
    w = at.worst_line
    end = sf[w] if at.from_end else st[w]
    mag = torch.sqrt(end.real * end.real + end.imag * end.imag)
    worst = mag if rating is None else mag / float(np.asarray(rating, dtype=np.float64)[w])
    return dict(p_from=sf.real, q_from=sf.imag, p_to=st.real, q_to=st.imag, p_inj=S.real, q_inj=S.imag, gen_p=gen_p, gen_q=gen_q,
                slack_p=slack_p, worst_loading=worst, v_min=v[at.v_min_bus], v_max=v[at.v_max_bus])


def loss(out, w):
    """sum_name w[name] . out[name] over the names of ``w`` that are not None (``out``: a dict or a ``Case``; torch or numpy)."""
    get = out.get if isinstance(out, dict) else (lambda name: getattr(out, name))
    total = 0.0
    for name in DIFF_OUT:
        if w.get(name) is None:
            continue
        weight, value = np.asarray(w[name], dtype=np.float64), get(name)
        if isinstance(value, torch.Tensor):
            total = total + (torch.as_tensor(weight) * value).sum()
        else:
            total = total + float(np.sum(weight * value))
    return total


def gradients(buses, lines, generators, slack_bus, v, theta, w, rating=None, at=None):
    """Float64 numpy gradients ``(buses [N,6], lines [E,7], generators [Gn,7], v [N], theta [N])`` of ``loss(outputs, w)`` at (v, theta),
    by torch autograd on the CPU; the summaries' indices are those of ``forward`` at this state unless ``at`` gives them."""
    if at is None:
        at = forward(buses, lines, generators, slack_bus, v, theta, rating)
    p = [torch.as_tensor(np.asarray(a, dtype=np.float64)).clone().requires_grad_(True) for a in (buses, lines, generators, v, theta)]
    total = loss(torch_outputs(*p, slack_bus, rating, at), w)
    grads = torch.autograd.grad(total, p, allow_unused=True)
    return [np.zeros(tuple(x.shape)) if g is None else g.numpy() for g, x in zip(grads, p)]

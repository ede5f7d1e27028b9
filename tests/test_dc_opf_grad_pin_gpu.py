"""GPU pins of ``gns_dcopf_adjoint_kernel`` (csrc/gns_dcopf_adjoint.hip) at KKT orders past a wave's 64 lanes, at the order the LDS
image caps, and on its rule and failure rows, on the sets of ``dc_opf_grad_pin_cases`` and the reused sets of ``dc_opf_pin_cases``.

Fed by the reference (``dc_opf_adjoint_call``): the kernel takes the float64 reference's optimum at 1e-11 as the forward's outputs,
so the forward's stopping tolerance does not enter; its gradient is compared with ``dc_opf_grad_reference.gradients`` at that same
point.  The bar follows ``dc_opf_pin_cases.iterate_bar``: per grid and input, ten times the gap between the two float64 references
(``dc_opf_grad_reference``: the full formulation; ``dc_opf_grad_reduced_reference``: the reduced algebra) plus ``DC_BAR = 1e-9`` at
the gradient's scale ``max(1, max|ref grad|)``, plus ``2^-24`` of the scale on the rows the kernel writes in float32 (``Pd``,
``Gs``, ``Pmax``, ``Pmin``).  Crafted tensors pin the strict ``>`` of the active-set rule, the zero pivot, the scans that decide
NaN rows and zero rows with the deciding element at an index of 64 or above, and the order that does not fit the image.

Through the public call: ``tests/test_dc_opf_grad_gpu.py``'s own ``_worst_ratio`` and bar (ten times the reference's move between
``tol`` and ``tol / 1000``, plus ``DC_BAR`` and the float32 rounding at the gradient's scale), unchanged.
Worst device error / bar per set, measured on an MI355X: ``profiles/dcopf_grad_pin/gpu_suite_summary.txt``."""
import numpy as np
import pytest
import torch

import dc_opf_adjoint_call as call
import dc_opf_cases as cases
import dc_opf_grad_pin_cases as gpin
import dc_opf_grad_reduced_reference as reduced
import dc_opf_grad_reference as gref
import dc_opf_pin_cases as pin
import dc_opf_reduced_reference as forward_reduced
import test_dc_opf_grad_gpu as base

pytestmark = pytest.mark.gpu
F32 = base.F32
ROWS32 = base.ROWS32
CRAFT = 'hub150_qp'                  # N = 150, E = 149, Gn = 70: every tensor has an index of 64 or above
G = 1                                # the grid of CRAFT the tensors are crafted on: it has free units past index 64 (grid 0 has none)
PUBLIC_SETS = tuple(n for n in gpin.SETS if n != 'cap_over') + tuple(pin.SETS)


# ---- fed by the reference

def _fed_bars(full, red):
    scale = max(1.0, max(np.abs(full[k]).max() for k in gref.INPUTS))
    return {k: 10.0 * np.abs(full[k] - red[k]).max() + cases.DC_BAR * scale + (F32 * scale if k in ROWS32 else 0.0) for k in gref.INPUTS}


def _fed_ratio(p, result, weights, grads, g, what):
    """The worst |device - reference| / bar of grid g of ``grads`` against both references' bar at ``result``, over all rows and over
    the float64 rows (``c2``, ``c1``, ``rating``) alone; asserts every one is <= 1."""
    full, red = gref.gradients(p, result, weights), reduced.gradients(p, result, weights)
    assert full['margin'] >= gref.MARGIN_MIN, (what, full['margin'])
    bars = _fed_bars(full, red)
    got = base._device_rows(grads, g, False, False)
    worst = np.zeros(2)
    for k, r in (('Pd', 'Pd'), ('Gs', 'Pd'), ('Pmax', 'Pmax'), ('Pmin', 'Pmin'), ('c2', 'c2'), ('c1', 'c1'), ('rating', 'rating')):
        err = np.abs(got[k] - full[r]).max()
        worst = np.maximum(worst, [err / bars[r], 0.0 if r in ROWS32 else err / bars[r]])
        assert err <= bars[r], (what, k, err, bars[r])
    assert np.all(got['rating'][~np.isfinite(p[4])] == 0.0)
    return worst


def _feed(name, weights, plant=None, **kw):
    """The direct call on a set, fed the reference's optimum at 1e-11 (``plant(outputs)`` changes the fed arrays in place first)."""
    b = cases.batch(name)
    outputs = call.stack(gpin.tight(name))
    if plant is not None:
        plant(outputs)
    Bt = b.buses.shape[0]
    incoming = {}
    for k in call.OUTPUTS:
        if any(w is not None and k in w for w in weights):
            shape = outputs[k].shape
            incoming[k] = np.stack([np.zeros(shape[1:]) if w is None or k not in w else np.broadcast_to(np.asarray(w[k], dtype=np.float64), shape[1:])
                                    for w in weights])
    assert len(weights) == Bt
    return call.adjoint(b, outputs, incoming, **kw)


@pytest.mark.parametrize('name', gpin.FED_SETS)
def test_adjoint_fed_by_the_reference(name):
    weights = gref.set_weights(name)
    grads = _feed(name, weights)
    worst = np.zeros(2)
    for g, (p, r) in enumerate(zip(cases.problems(name), gpin.tight(name))):
        if name == 'cap_over' and g == 0:            # order 131 against a cap of 130: NaN rows, from the fed tensors alone
            assert base._all_nan(grads, 0)
            continue
        worst = np.maximum(worst, _fed_ratio(p, r, weights[g], grads, g, (name, g)))
    print(f'DCOPF_GRAD_PIN_SUMMARY fed {name}: worst error / bar {worst[0]:.3f} (float64 rows {worst[1]:.3f})')


# ---- the rule and the failure rows on crafted tensors

def _craft_places():
    """On grid G of CRAFT at the fed point: an inactive rated line, a second one, a line without a rating and a free unit, each at
    the largest index (64 or above: asserted)."""
    p, r = cases.problems(CRAFT)[G], gpin.tight(CRAFT)[G]
    state, row, _ = reduced.active_set(p, r)
    rated = np.flatnonzero(np.isfinite(p[4]) & (row == 0))
    unrated = np.flatnonzero(~np.isfinite(p[4]))
    free = np.flatnonzero(state == 0)
    assert rated.size >= 2 and rated[-2] >= 64 and unrated[-1] >= 64 and free[-1] >= 64
    assert (row != 0).sum() >= 1 and (state != 0).sum() >= 1
    return int(rated[-1]), int(rated[-2]), int(unrated[-1]), int(free[-1])


def test_ties_are_not_active_and_a_line_without_a_rating_never_is():
    """``mu_line == rating - flow``, ``-mu_line == rating + flow`` and ``mu_pmax == Pmax - p`` at elements 64 or above: the rule is a
    strict ``>``, so the gradient keeps the untied feed's bits; one ulp above the tie it does not.  A line with ``rating = inf``
    stays out whatever its ``mu_line``."""
    weights = gref.set_weights(CRAFT)
    clean = _feed(CRAFT, weights)
    l_up, l_down, l_inf, q = _craft_places()
    p = cases.problems(CRAFT)[G]
    rating, pmax = p[4], p[2][:, 1]

    def tie(o, ulps=0):
        o['mu_line'][G, l_up] = rating[l_up] - o['line_flow'][G, l_up]
        o['mu_line'][G, l_down] = 0.0 - (rating[l_down] + o['line_flow'][G, l_down])
        o['mu_pmax'][G, q] = pmax[q] - o['pg'][G, q]
        o['mu_line'][G, l_inf] = 1e6
        for _ in range(ulps):
            o['mu_line'][G, l_up] = np.nextafter(o['mu_line'][G, l_up], np.inf)

    tied = _feed(CRAFT, weights, tie)
    assert base._same_bits(base._grad_list(clean), base._grad_list(tied))
    above = _feed(CRAFT, weights, lambda o: tie(o, 1))
    assert not base._same_bits(base._grad_list(clean, [G]), base._grad_list(above, [G]))      # the tied element is read
    assert base._same_bits(base._grad_list(clean, [1 - G]), base._grad_list(above, [1 - G]))


def test_a_zero_pivot_gives_nan_rows_and_leaves_the_neighbour_alone():
    """Two units with ``c2 = 0``, both fed as free, no line active: K = [[0,0,1],[0,0,1],[1,1,0]], whose second pivot is exactly 0."""
    name = 'path66_pv'
    b = cases.batch(name)
    assert b.gens.shape[1] == 2 and b.cost.dim() == 3
    cost = b.cost.clone()
    cost[0, :, 0] = 0.0
    b = b._replace(cost=cost)
    outputs = call.stack(gpin.tight(name))
    outputs['pg'][0] = 0.5 * (b.gens[0, :, 1] + b.gens[0, :, 2]).double().numpy()
    for k in ('mu_line', 'mu_pmax', 'mu_pmin'):
        outputs[k][0] = 0.0
    weights = gref.set_weights(name)
    incoming = {k: np.stack([np.asarray(w[k], dtype=np.float64) for w in weights]) for k in call.OUTPUTS}
    grads = call.adjoint(b, outputs, incoming)
    assert base._all_nan(grads, 0)
    assert all(bool(torch.isfinite(t[1]).all()) for t in base._grad_list(grads))
    one = cases.Batch(b.buses[1:], b.lines[1:], b.gens[1:], b.cost[1:].contiguous(), b.rating[1:].contiguous(), b.slack)
    alone = call.adjoint(one, {k: v[1:] for k, v in outputs.items()}, {k: v[1:] for k, v in incoming.items()})
    assert base._same_bits(base._grad_list(grads, [1]), base._grad_list(alone))


PLANTS = call.OUTPUTS + ('converged', 'iterations')


@pytest.mark.parametrize('what', PLANTS)
def test_a_nan_output_or_a_failed_forward_gives_nan_rows_for_that_grid_only(what):
    """A NaN at the last element of one output of grid 1 (index 64 or above in every output but the objective), ``converged = 0``
    or ``iterations = -1``: NaN rows there, grid 0's bits unchanged."""
    weights = gref.set_weights(CRAFT)
    clean = _feed(CRAFT, weights)
    kw = {}
    plant = None
    if what == 'converged':
        kw['converged'] = [1, 0]
    elif what == 'iterations':
        kw['iterations'] = [9, -1]
    else:
        def plant(o):
            if what == 'objective':
                o[what][1] = np.nan
            else:
                assert o[what].shape[1] - 1 >= 64
                o[what][1, -1] = np.nan
    grads = _feed(CRAFT, weights, plant, **kw)
    assert base._all_nan(grads, 1)
    assert base._same_bits(base._grad_list(clean, [0]), base._grad_list(grads, [0]))
    assert all(bool(torch.isfinite(t[0]).all()) for t in base._grad_list(grads))


@pytest.mark.parametrize('output', ('theta', 'line_flow', 'pg'))
def test_one_cotangent_element_past_the_first_wave_is_seen(output):
    """The cotangent is zero but for one element of one output of grid G, at an index of 64 or above (of ``pg``: the last free unit,
    so that it passes through the KKT solve): the rows are not zero and match the reference; the other grid, where nothing comes
    in, gets zero rows."""
    p, r = cases.problems(CRAFT)[G], gpin.tight(CRAFT)[G]
    size = np.asarray(r[output]).size
    if output == 'pg':
        i = _craft_places()[3]
    elif output == 'line_flow':          # the last line whose flow depends on the dispatch, so that the cotangent passes through the solve
        i = int(np.flatnonzero(np.abs(forward_reduced.model(*p)['S']).max(axis=1) > 1e-3)[-1])
    else:
        i = size - 1
    assert i >= 64 and (output != 'theta' or p[5] != i + 1)          # (not the slack's angle: it is 0 whatever the data)
    w = np.zeros(size)
    w[i] = 1.0
    weights = [None, None]
    weights[G] = {output: w}
    grads = _feed(CRAFT, weights)
    assert bool((grads['buses'][G] != 0).any()) and bool((grads['cost'][G] != 0).any()) and base._all_zero(grads, 1 - G)
    worst = _fed_ratio(p, r, weights[G], grads, G, (output, i))
    print(f'DCOPF_GRAD_PIN_SUMMARY one-element {output}[{i}] {CRAFT}: worst error / bar {worst[0]:.3f} (float64 rows {worst[1]:.3f})')


def test_no_cotangent_gives_zero_rows_whatever_the_grid_holds():
    """All cotangents zero (given as zeros, not left out) and a NaN in an output: the zero test comes first."""
    zeros = {k: 0.0 for k in call.OUTPUTS}

    def plant(o):
        o['theta'][1, -1] = np.nan
        o['mu_pmax'][0, -1] = np.nan
    grads = _feed(CRAFT, [zeros, zeros], plant, converged=[0, 1], iterations=[9, -1])
    assert base._all_zero(grads, 0) and base._all_zero(grads, 1)
    weights = gref.set_weights(CRAFT)
    clean = _feed(CRAFT, weights)

    def plant_one(o):
        o['theta'][1, -1] = np.nan
    grads = _feed(CRAFT, [weights[0], {k: np.zeros_like(v) for k, v in weights[1].items()}], plant_one)
    assert base._all_zero(grads, 1) and base._same_bits(base._grad_list(clean, [0]), base._grad_list(grads, [0]))


# ---- through the public call

@pytest.mark.parametrize('name', PUBLIC_SETS)
def test_public_gradient_against_the_reference(name):
    worst = base._worst_ratio(name, gref.set_weights(name))
    print(f'DCOPF_GRAD_PIN_SUMMARY public {name}: worst error / bar {worst:.3f}')


def test_forward_converges_on_every_new_set():
    for name in gpin.SETS:
        res, _ = base._run(cases.batch(name), None)
        print(f'DCOPF_GRAD_PIN_SUMMARY forward {name}: iterations {res.iterations.tolist()}')
        assert bool(res.converged.all()), (name, res.iterations.tolist())


def test_the_order_above_the_cap_gives_nan_rows_through_the_public_call():
    """``cap_over``: grid 0's system has order 131 on a cap of 130 (NaN in all four gradient tensors); grid 1's fits: within the
    bar, and bit-identical to its run alone.  With the loss indexing grid 0 out, grid 0's rows are zero."""
    name = 'cap_over'
    b = cases.batch(name)
    weights = gref.set_weights(name)
    assert gref.kept_grids(name)[0] == (0, 1)
    res, grads = base._run(b, weights)
    assert bool(res.converged.all())
    assert len([t for t in base._grad_list(grads) if t is not None]) == 4 and base._all_nan(grads, 0)
    ref_g, bars = base._reference(name, weights)[1]
    got = base._device_rows(grads, 1, False, False)
    worst = 0.0
    for k, r in (('Pd', 'Pd'), ('Gs', 'Pd'), ('Pmax', 'Pmax'), ('Pmin', 'Pmin'), ('c2', 'c2'), ('c1', 'c1'), ('rating', 'rating')):
        err = np.abs(got[k] - ref_g[r]).max()
        worst = max(worst, err / bars[r])
        assert err <= bars[r], (k, err, bars[r])
    print(f'DCOPF_GRAD_PIN_SUMMARY public {name}: worst error / bar {worst:.3f}')
    one = cases.Batch(b.buses[1:], b.lines[1:], b.gens[1:], b.cost[1:].contiguous(), b.rating[1:].contiguous(), b.slack)
    _, alone = base._run(one, weights[1:])
    assert base._same_bits(base._grad_list(grads, [1]), base._grad_list(alone))
    _, out = base._run(b, [None, weights[1]])
    assert base._all_zero(out, 0) and base._same_bits(base._grad_list(grads, [1]), base._grad_list(out, [1]))


@pytest.mark.parametrize('name', ('free64', 'free70_lines'))
def test_bits_alone_in_a_batch_reversed_and_again(name):
    base.test_forward_bits_and_gradient_alone_in_a_batch_reversed_and_again(name)

"""CPU side of the DC OPF adjoint's pins (``tests/test_dc_opf_grad_pin_gpu.py``), no device needed: what the sets of
``dc_opf_grad_pin_cases`` promise (``check()``: the KKT orders 63, 64, 65 and 74, the order at the LDS cap and one above, from the
float64 reference and from the library's host queries); which grids of the reused sets of ``dc_opf_pin_cases`` have a derivative
(margin at least ``MARGIN_MIN = 1e-4``), stated literally; the second float64 reference (``dc_opf_grad_reduced_reference``, the
reduced algebra) against the full one on every set, the gap the fed tests' bars are built from, and against central differences;
and that ``dc_opf_grad_reference.set_weights`` still gives the sets of ``dc_opf_cases.SETS`` the weights it gave them."""
import numpy as np
import pytest

import dc_opf_cases as cases
import dc_opf_grad_pin_cases as gpin
import dc_opf_grad_reduced_reference as reduced
import dc_opf_grad_reference as gref
import dc_opf_pin_cases as pin

FD_BAR, FD_STEP = 1e-6, 1e-5         # tests/test_dc_opf_grad_host.py's
EXCLUDED = [('gn40', 1)]             # the grids of dc_opf_pin_cases without a derivative worth comparing


def test_the_sets_keep_their_promises():
    out = gpin.check()
    for name, rows in out.items():
        print(name, ' '.join(f'[nf {nf} k {k} n {n} margin {m:.1e}]' for nf, k, n, m in rows))
    assert gpin.draw_lines() == gpin.LINES_DRAW            # the constant is the search's answer
    assert gpin.lds_queries(gpin.CAP - 1)[1:] == (163464, gpin.CAP)      # n = 130 fills the image to 376 bytes under the limit


def test_kept_and_excluded_grids_stated_literally():
    assert gref.MARGIN_MIN == 1e-4
    margins = {name: gref.kept_grids(name)[1] for name in pin.SETS}
    for name, ms in margins.items():
        print(name, ' '.join(f'{m:.1e}' for m in ms))
    assert sum(len(m) for m in margins.values()) == 26
    assert [(name, g) for name in pin.SETS for g, m in enumerate(margins[name]) if m < gref.MARGIN_MIN] == EXCLUDED
    for name in gpin.REUSED:
        assert gref.kept_grids(name)[0] == (0, 1), name
    for name in gpin.SETS:                            # every grid of every new set is kept: asserted, not filtered
        assert gref.kept_grids(name)[0] == (0, 1), name
        assert all(m >= gref.MARGIN_MIN for *_, m in gpin.orders(name))
    assert set(gpin.FED_SETS) == set(gpin.SETS) | set(gpin.REUSED) | {'hub150_lp'}


def test_the_reused_sets_reach_orders_past_a_wave():
    """What the fed tests run on besides the new sets: KKT orders 74/56, 84/71, 73/59 on gn63, gn64, gn65 and an active line at
    index 64 or above next to six units on mixed_ratings; a lower limit active, a unit at Pmin and one at Pmax over the others."""
    n = {name: [o[2] for o in gpin.orders(name)] for name in ('gn63', 'gn64', 'gn65')}
    print(n)
    assert all(max(v) > 64 for v in n.values())
    top, lower, at_min, at_max = 0, 0, 0, 0
    for name in gpin.REUSED:
        for p, r in zip(cases.problems(name), gpin.tight(name)):
            state, row, _ = reduced.active_set(p, r)
            if name == 'mixed_ratings':
                top = max(top, int(np.flatnonzero(row != 0).max()))
            lower, at_min, at_max = lower + int((row < 0).sum()), at_min + int((state == 2).sum()), at_max + int((state == 1).sum())
    assert top >= 64 and lower >= 1 and at_min >= 1 and at_max >= 1, (top, lower, at_min, at_max)


ALL_SETS = tuple(gpin.SETS) + tuple(pin.SETS) + tuple(cases.SETS)


@pytest.mark.parametrize('name', ALL_SETS)
def test_reduced_reference_against_the_full_one(name):
    """The same active set, the same margin and the same gradient from two formulations that share no algebra.  The gap printed
    here is the yardstick of the fed tests' bars; it stays below the project's DC bar at the gradient's scale."""
    weights = gref.set_weights(name)
    for g in gref.kept_grids(name)[0]:
        p, r = cases.problems(name)[g], gpin.tight(name)[g]
        a, b = gref.gradients(p, r, weights[g]), reduced.gradients(p, r, weights[g])
        state, row, _ = reduced.active_set(p, r)
        nf, k, _ = gpin.counts(p, r)
        assert (int((state == 0).sum()), int((row != 0).sum())) == (nf, k)
        assert abs(a['margin'] - b['margin']) <= 1e-12
        scale = max(1.0, max(np.abs(a[key]).max() for key in gref.INPUTS))
        gap = max(np.abs(a[key] - b[key]).max() for key in gref.INPUTS)
        print(f'{name}[{g}] n {nf + 1 + k} scale {scale:.2e} |reduced - full| / scale {gap / scale:.2e}')
        assert gap <= cases.DC_BAR * scale, (name, g, gap, scale)


@pytest.mark.parametrize('name', ('free62', 'gn5'))
def test_reduced_reference_against_central_differences(name):
    weights = gref.set_weights(name)
    for g in gref.kept_grids(name)[0]:
        p, r = cases.problems(name)[g], gpin.tight(name)[g]
        grads = reduced.gradients(p, r, weights[g])
        scale = max(1.0, max(np.abs(grads[k]).max() for k in gref.INPUTS))
        worst = 0.0
        for k in gref.INPUTS:
            idx = np.flatnonzero(np.isfinite(p[4])) if k == 'rating' else np.arange(grads[k].size)
            for i in sorted({int(j) for j in idx[[0, -1]]}):
                fd = gref.central_difference(p, weights[g], k, i, FD_STEP)
                worst = max(worst, abs(fd - grads[k][i]) / scale)
                assert abs(fd - grads[k][i]) <= FD_BAR * scale, (name, g, k, i, fd, grads[k][i], scale)
        print(f'{name}[{g}] scale {scale:.2e} worst |fd - reduced| / scale {worst:.2e}')


def test_set_weights_keeps_the_old_sets_bits_and_places_the_new_ones_past_them():
    name = 'case14_qp'
    place = sorted(cases.SETS).index(name)
    for g, (p, w) in enumerate(zip(cases.problems(name), gref.set_weights(name))):
        want = gref.random_weights(p, np.random.default_rng([20, place, g]))
        assert all(w[k].tobytes() == want[k].tobytes() for k in gref.OUTPUTS)
    w = gref.set_weights(name)[0]
    assert (w['pg'][0].hex(), float(w['objective']).hex()) == WEIGHT_BITS
    assert not set(cases.OTHER_SETS) & set(cases.SETS)
    for name, crc in (('free64', 0x6319571), ('gn63', 0xf33006ef)):            # zlib.crc32 of the name: a place no later set moves
        p = cases.problems(name)[1]
        want = gref.random_weights(p, np.random.default_rng([20, len(cases.SETS) + crc, 1]))
        got = gref.set_weights(name)[1]
        assert all(got[k].tobytes() == want[k].tobytes() for k in gref.OUTPUTS)
    only = gref.set_weights('free64', only='lmp')[0]
    assert list(only) == ['lmp'] and only['lmp'].tobytes() == gref.set_weights('free64')[0]['lmp'].tobytes()


WEIGHT_BITS = ('0x1.4d3e0b47ba012p-1', '0x1.71ba26a7e3c28p-1')      # case14_qp grid 0: pg[0] and objective, as the parent drew them

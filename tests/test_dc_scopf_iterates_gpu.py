"""GPU checks of the path ``powerflow.dc_security_constrained_opf`` takes and of its row slots, not only of where it ends
(include/gns_powerflow.h, "Security-constrained DC optimal power flow"): the start (``max_iter = 0``), the iterate after 1, 2 and 3
updates against ``dc_scopf_reference.solve`` (dense float64 numpy, every row from the network rebuilt without its outaged line), the
iteration count, bit-identity across layouts of one list, and the sets of ``dc_scopf_pin_cases`` (lists with live rows at and past
slot 63, holes at the trips' edges, duplicates, rows on unrated lines, a narrow row chunk) through the checks of
``tests/test_dc_scopf_gpu.py``.  An interior point corrects itself: a wrong normal matrix, gamma, step length or a row dropped at
a wave edge still reaches an optimum that the end-point checks accept or nearly accept; these tests look at the path.

Bars.  The start: the project's DC bar ``1e-9 max(1, max|ref|)``.  An iterate: ten times the set's yardstick at that k (how far the
reduced and the full float64 reference are apart there, ``dc_scopf_pin_cases.yardstick``, computed on the CPU over pg, mu_line,
mu_row, mu_pmax, mu_pmin) plus the DC bar, at the scale of the reference's value (``dc_scopf_pin_cases.iterate_bar``).  The count:
equal, on every grid run alone at the tolerance ``dc_scopf_pin_cases.count_at`` picks for it, where no figure of the reference's
run is within a factor 2.2 of the tolerance; at the default tolerance equal, or off by one on a near tie.

Measured: yardstick (CPU) and the device's worst difference on an MI355X, both relative (``max|a - b| / max(1, max|ref|)``, the
largest over the grids; the yardstick over pg, mu_line, mu_row, mu_pmax, mu_pmin, the device also over objective, lmp and row_flow
at the live slots), per set and k:

    set                yardstick k = 0 / 1 / 2 / 3                 device k = 0 / 1 / 2 / 3
    three_bus          0.0e+00 / 4.4e-16 / 7.7e-12 / 9.9e-14       0.0e+00 / 4.3e-16 / 5.3e-14 / 1.0e-15
    case14_qp          1.2e-15 / 6.3e-14 / 1.0e-12 / 2.8e-11       2.7e-15 / 5.1e-15 / 1.8e-13 / 1.9e-11
    case14_lp          6.7e-16 / 4.3e-14 / 4.5e-13 / 1.4e-11       9.7e-16 / 1.2e-15 / 5.2e-13 / 2.3e-11
    meshed14           4.4e-16 / 4.0e-14 / 2.3e-13 / 1.0e-11       3.9e-15 / 3.1e-15 / 1.8e-14 / 3.5e-13
    stacked_units      5.6e-16 / 4.1e-14 / 3.2e-13 / 5.3e-10       5.7e-15 / 4.2e-15 / 3.0e-14 / 3.7e-11
    ring30             2.1e-15 / 1.6e-14 / 1.7e-12 / 3.9e-10       3.8e-15 / 9.9e-15 / 6.0e-13 / 2.0e-11
    lattice5           1.0e-15 / 1.3e-13 / 7.0e-13 / 4.6e-10       3.0e-15 / 8.9e-15 / 2.4e-13 / 2.8e-11
    wheel_qp_r63       0.0e+00 / 2.1e-13 / 1.0e-13 / 1.3e-11       2.1e-14 / 2.0e-14 / 9.9e-13 / 1.3e-11
    wheel_qp_r64       0.0e+00 / 1.6e-13 / 1.2e-12 / 2.5e-11       2.9e-14 / 2.3e-14 / 5.0e-13 / 2.2e-11
    wheel_lp_r65       0.0e+00 / 1.2e-13 / 1.3e-12 / 1.7e-11       1.4e-14 / 1.3e-14 / 2.0e-12 / 8.6e-11
    live64             7.8e-16 / 1.9e-13 / 3.1e-11 / 5.9e-12       2.8e-15 / 3.1e-15 / 2.7e-12 / 1.4e-12
    live65             1.0e-15 / 4.3e-14 / 3.1e-13 / 3.2e-11       2.5e-15 / 2.1e-15 / 8.0e-13 / 3.5e-12
    live128            2.3e-15 / 1.6e-13 / 4.5e-11 / 5.7e-11       5.5e-15 / 4.7e-15 / 3.4e-11 / 2.9e-11
    live129            2.3e-15 / 3.9e-14 / 2.0e-12 / 1.4e-12       2.9e-15 / 3.3e-15 / 4.9e-13 / 8.0e-13
    edge_holes         7.8e-16 / 1.3e-13 / 5.9e-13 / 4.8e-12       2.5e-15 / 3.6e-15 / 8.5e-14 / 3.3e-13
    shared_rows        3.3e-16 / 9.5e-14 / 1.6e-12 / 4.7e-12       2.7e-15 / 2.1e-15 / 1.4e-12 / 7.5e-12
    unrated_monitored  5.6e-16 / 2.6e-13 / 6.6e-13 / 2.3e-11       1.4e-15 / 4.2e-15 / 2.6e-13 / 2.6e-11
    listed_unrated_c   6.7e-16 / 6.0e-14 / 5.8e-13 / 8.4e-13       3.4e-15 / 3.5e-15 / 2.9e-14 / 2.1e-12
    narrow_rows        1.0e-13 / 8.8e-13 / 1.1e-12 / 1.0e-11       1.0e-13 / 2.4e-13 / 4.1e-13 / 7.3e-12
    loose_rows         2.8e-16 / 7.1e-14 / 1.3e-13 / 2.9e-11       4.3e-15 / 3.5e-15 / 2.6e-13 / 8.7e-12

Every bar above is (10 yardstick + 1e-9), so the device stays a factor of 13 or more inside it.  Run alone at its own tolerance
every one of the 40 grids stops at the reference's count; at the default tolerance the counts are equal on all 40 too, the 26
near ties included.
"""
import numpy as np
import pytest
import torch

import dc_opf_reduced_reference as red
import dc_reference
import dc_scopf_cases as cases
import dc_scopf_pin_cases as pin
import dc_scopf_reference as ref
import test_dc_scopf_gpu as base

pytestmark = pytest.mark.gpu
COMPARED = ('pg', 'mu_line', 'mu_row', 'mu_pmax', 'mu_pmin', 'objective', 'lmp')
EARLY = (1, 2, 3)

_AT = {}


def _at(name, k):
    """The device's result on a set after at most k updates, computed once and left unchanged."""
    if (name, k) not in _AT:
        _AT[name, k] = base._run(cases.case(name), max_iter=k)
        torch.cuda.synchronize()
    return _AT[name, k]


def _dc_bar(want):
    return cases.DC_BAR * max(1.0, float(np.abs(want).max()))


def _rel(got, want):
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


def _check_theta_and_flows(res, name):
    """theta and line_flow are the DC power flow at the returned dispatch, whatever the iterate."""
    for g, (p, _) in enumerate(cases.problems(name)):
        r = base._grid(res, g)
        gens = p[2].copy()
        gens[:, 6] = r['pg']
        theta, flow, _ = dc_reference.dc_power_flow(torch.from_numpy(p[0]), torch.from_numpy(p[1]), torch.from_numpy(gens), p[5])
        for got, want in ((r['theta'], theta.numpy()), (r['line_flow'], flow.numpy())):
            assert np.abs(got - want).max() <= _dc_bar(want), (name, g)


def _dead(rows, rc):
    dead = np.ones(rows.shape[0], dtype=bool)
    dead[pin.live_slots(rows, rc)] = False
    return dead


@pytest.mark.parametrize('name', pin.ALL_SETS)
def test_the_start(name):
    res, b = _at(name, 0), cases.case(name).batch
    Bt = b.buses.shape[0]
    assert res.iterations.tolist() == [0] * Bt and not bool(res.converged.any())
    assert torch.equal(res.pg.cpu(), 0.5 * (b.gens[:, :, 1].double() + b.gens[:, :, 2].double()))
    worst = 0.0
    for g, ((p, rc, rows), want) in enumerate(zip(pin.grids(name), pin.iterates(name, 0))):
        r = base._grid(res, g)
        live, dead = pin.live_slots(rows, rc), _dead(rows, rc)
        pmid, flow, lim = 0.5 * (p[2][:, 1] + p[2][:, 2]), want['line_flow'], np.isfinite(p[4])
        # the rows' flows at the midpoint from the rebuilt networks: the ratings play no part, this is L_r by itself
        f = ref.row_values(p[0], p[1], p[2], p[5], rows, pmid)[0][live]
        assert np.abs(r['row_flow'][live] - f).max() <= _dc_bar(f), (name, g, 'row_flow')
        assert np.all(np.isnan(r['row_flow'][dead])) and np.all(r['mu_row'][dead] == 0.0), (name, g)
        # the start rule, written out: mu = 1 / z with z = max(1, -h) at the midpoint, lambda = 0
        rcl = rc[rows[live, 0]]
        mu_row, mu_line = np.zeros(rows.shape[0]), np.zeros(lim.size)
        mu_row[live] = 1.0 / np.maximum(1.0, rcl - f) - 1.0 / np.maximum(1.0, rcl + f)
        mu_line[lim] = 1.0 / np.maximum(1.0, p[4][lim] - flow[lim]) - 1.0 / np.maximum(1.0, p[4][lim] + flow[lim])
        rule = dict(mu_row=mu_row, mu_line=mu_line, mu_pmax=1.0 / np.maximum(1.0, p[2][:, 1] - pmid),
                    mu_pmin=1.0 / np.maximum(1.0, pmid - p[2][:, 2]), objective=np.float64(p[3][:, 0] @ pmid ** 2 + p[3][:, 1] @ pmid))
        assert want['lam'] == 0.0
        for k, v in rule.items():
            assert np.abs(want[k] - v).max() <= 1e-13 * max(1.0, np.abs(v).max()), (name, g, k)      # the reference obeys it
            assert np.abs(r[k] - v).max() <= _dc_bar(v), (name, g, k)
        assert np.all(r['mu_line'][~lim] == 0.0)
        assert np.abs(r['lmp'] - want['lmp']).max() <= _dc_bar(want['lmp']), (name, g)
        worst = max([worst] + [_rel(r[k], want[k]) for k in COMPARED] + [_rel(r['row_flow'][live], want['row_flow'][live])])
    print(f'PIN {name} k 0 yardstick {pin.yardstick(name, 0):.1e} device {worst:.1e}')
    _check_theta_and_flows(res, name)


@pytest.mark.parametrize('k', EARLY)
@pytest.mark.parametrize('name', pin.ALL_SETS)
def test_the_iterate_after_k_updates(name, k):
    res = _at(name, k)
    Bt = res.pg.shape[0]
    assert res.iterations.tolist() == [k] * Bt and not bool(res.converged.any())
    worst, over = 0.0, []
    for g, ((p, rc, rows), want) in enumerate(zip(pin.grids(name), pin.iterates(name, k))):
        r = base._grid(res, g)
        live, dead = pin.live_slots(rows, rc), _dead(rows, rc)
        assert np.all(np.isnan(r['row_flow'][dead])) and np.all(r['mu_row'][dead] == 0.0), (name, g)
        pairs = [(key, r[key], want[key]) for key in COMPARED] + [('row_flow', r['row_flow'][live], want['row_flow'][live])]
        for key, got, ref_value in pairs:
            diff, bar = float(np.abs(got - ref_value).max()), pin.iterate_bar(name, k, ref_value)
            worst = max(worst, _rel(got, ref_value))
            if not diff <= bar:
                over.append((g, key, diff, bar))
    print(f'PIN {name} k {k} yardstick {pin.yardstick(name, k):.1e} device {worst:.1e}')
    assert not over, (name, k, over)
    _check_theta_and_flows(res, name)


@pytest.mark.parametrize('name', pin.ALL_SETS)
def test_the_iteration_count_where_no_tie_exists(name):
    """Every grid alone (a grid's result is bit-identical alone) at its own tolerance: the reference's count, no exception."""
    c = base._per_grid(cases.case(name))
    wrong = []
    for g, (tol, ratio, count) in enumerate(pin.count_at(name)):
        got = base._run(base._take(c, [g]), tol=tol)
        print(f'COUNT {name}[{g}] tol {tol:.3e} (nearest figure a factor {ratio:.2f} away) device {int(got.iterations[0])} reference {count}')
        assert bool(got.converged[0]), (name, g)
        if int(got.iterations[0]) != count:
            wrong.append((g, int(got.iterations[0]), count))
    assert not wrong, (name, wrong)


@pytest.mark.parametrize('name', pin.ALL_SETS)
def test_the_iteration_count_at_the_default_tolerance(name):
    """``test_dc_opf_iterates_gpu``'s rule: equal, or off by one where the reference's run is a near tie."""
    res = base._result(name)
    wrong, ties = [], 0
    for g, want in enumerate(cases.optimum(name)):
        got, tie = int(res.iterations[g]), red.near_tie(want['figures'])
        ties += tie
        print(f"COUNT {name}[{g}] device {got} reference {want['iterations']}" + (' (near tie)' if tie else ''))
        assert bool(res.converged[g]) and want['converged']
        if abs(got - want['iterations']) > (1 if tie else 0):
            wrong.append((g, got, want['iterations'], tie))
    print(f'NEAR TIES {name} {ties} of {len(cases.optimum(name))}')
    assert not wrong, (name, wrong)


@pytest.mark.parametrize('k', (2, ref.DEFAULT_MAX_ITER))
def test_edge_holes_packed_to_the_front_is_the_same_bits(k):
    """The live rows are placed in list order and every sum over rows runs over the live rows in list order: where the holes are
    changes no bit of the ten base fields, nor of mu_row and row_flow at the live slots.  The packed list has R = 125, grid 0's
    live count; grid 1 has one row fewer and so an empty last slot."""
    c = cases.case('edge_holes')
    live = [torch.from_numpy(pin.live_slots(rows, rc)) for _, rc, rows in pin.grids('edge_holes')]
    n = max(len(s) for s in live)
    packed = torch.full((2, n, 2), -1, dtype=torch.int32)
    for g, s in enumerate(live):
        packed[g, :len(s)] = c.rows[g, s]
    a, b = base._run(c, max_iter=k), base._run(c, rows=packed, max_iter=k)
    assert k > 3 or a.iterations.tolist() == [k, k]
    assert bool(a.converged.all()) == (k > 3)
    assert base._same_bits(list(a)[:10], list(b)[:10])
    for g, s in enumerate(live):
        s = s.to(a.mu_row.device)
        assert base._same_bits([a.mu_row[g, s], a.row_flow[g, s]], [b.mu_row[g, :len(s)], b.row_flow[g, :len(s)]]), g
        assert bool((b.mu_row[g, len(s):] == 0).all()) and bool(torch.isnan(b.row_flow[g, len(s):]).all())


@pytest.mark.parametrize('k', (2, ref.DEFAULT_MAX_ITER))
def test_a_listed_row_without_a_contingency_rating_is_an_empty_slot_bit_for_bit(k):
    """``listed_unrated_c``'s rows on lines whose contingency rating is +inf (slots 1, 63, 64) against (-1, -1) there."""
    c = cases.case('listed_unrated_c')
    rows = c.rows.clone()
    for s in pin.UNRATED_C_SLOTS:
        assert bool((rows[:, s] >= 0).all())
        rows[:, s] = -1
    a, b = base._run(c, max_iter=k), base._run(c, rows=rows, max_iter=k)
    assert base._same_bits(a, b)
    for s in pin.UNRATED_C_SLOTS:
        assert bool((a.mu_row[:, s] == 0).all()) and bool(torch.isnan(a.row_flow[:, s]).all())


def test_live129_after_two_updates_is_bit_identical_alone_in_a_batch_reversed_and_shared():
    name, k = 'live129', 2
    c = cases.case(name)
    assert c.rows.shape == (2, 129, 2) and c.batch.cost.dim() == 3 and c.rating_c.dim() == 2
    whole = _at(name, k)
    assert whole.iterations.tolist() == [k, k]
    assert base._same_bits(whole, base._run(c, max_iter=k))
    assert base._same_bits([t[[1, 0]] for t in whole], base._run(base._take(c, [1, 0]), max_iter=k))
    for g in range(2):
        assert base._same_bits([t[g:g + 1] for t in whole], base._run(base._take(c, [g]), max_iter=k))
    # one list for both grids (grid 0's: every row with a finite contingency rating is feasible on both) against a copy per grid
    shared = base._run(c, rows=c.rows[0].contiguous(), max_iter=k)
    assert base._same_bits(shared, base._run(c, rows=torch.stack([c.rows[0], c.rows[0]]), max_iter=k))
    assert base._same_bits([t[0:1] for t in shared], [t[0:1] for t in whole])


@pytest.mark.parametrize('k', pin.KS)
def test_duplicates_carry_equal_multipliers_bit_for_bit(k):
    """At the optimum the multipliers of two identical rows are not unique (only the KKT certificate judges them there); the
    iterates are, because identical rows stay equal."""
    res = _at('shared_rows', k)
    rows = [tuple(r) for r in cases.case('shared_rows').rows.tolist()]
    dup = [[i for i, r in enumerate(rows) if r == d] for d in sorted(set(rows)) if rows.count(d) > 1]
    assert len(dup) >= 2
    for i, j in dup:
        assert base._same_bits([res.mu_row[:, i], res.row_flow[:, i]], [res.mu_row[:, j], res.row_flow[:, j]]), (k, i, j)
        assert k == 0 or bool((res.mu_row[:, i] != 0).all())      # (at the start a row with both slacks at 1 has mu_row = 0 exactly)


@pytest.mark.parametrize('name', tuple(pin.SETS))
def test_the_new_sets_through_the_existing_checks(name):
    """The optimum against the reference, the flows, the rows and the KKT certificate, every slot empty."""
    base.test_optimum_against_the_reference(name)
    base.test_flows_rows_and_the_kkt_certificate(name)
    base.test_every_slot_empty_is_dc_optimal_power_flow_bit_for_bit(name)

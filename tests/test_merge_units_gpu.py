"""Replica merge that carries units (m3gpu_merge_batch_units_dev): every
emitted point gets the unit of the replica whose value it got. Each replica's
points carry a unit that names the replica, the expectation is the Python
restatement of the winner rule that test_decode_full_cpu.py checks against
the oracle, and ts, vals, counts and errs equal m3gpu_merge_batch_dev's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_full_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A
USENT = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    t.cuda.set_device(DEV)
    return t


@pytest.fixture(scope="module")
def engine():
    from m3_amd import engine as e
    return e


@pytest.mark.parametrize("out_stride_odd", [False, True])
@pytest.mark.parametrize("R", [1, 2, 4])
def test_merge_carries_the_winners_unit(torch, engine, R, out_stride_odd):
    ts, vals, units, counts = cases.merge_inputs(R)
    _, nseries, stride = ts.shape
    model = cases.merge_model(ts, vals, units, counts)
    out_stride = max(len(m[0]) for m in model) + (1 if out_stride_odd else 2)
    d_ts = torch.from_numpy(ts.reshape(R * nseries, stride)).to(DEV)
    d_vals = torch.from_numpy(vals.reshape(R * nseries, stride)).to(DEV)
    d_units = torch.from_numpy(units.reshape(R * nseries, stride)).to(DEV)
    d_counts = torch.from_numpy(counts.reshape(-1).astype(np.int32)).to(DEV)

    def outputs():
        return (torch.full((nseries + 1, out_stride), SENTINEL,
                           dtype=torch.int64, device=DEV),
                torch.full((nseries + 1, out_stride), SENTINEL,
                           dtype=torch.int64, device=DEV).view(torch.float64),
                torch.full((nseries,), -1, dtype=torch.int32, device=DEV),
                torch.full((nseries,), -1, dtype=torch.int32, device=DEV))

    u_ts, u_vals, u_counts, u_errs = outputs()
    # unit rows at an odd address, guard bytes in front, a guard row behind
    flat_u = torch.full((3 + (nseries + 1) * out_stride,), USENT,
                        dtype=torch.uint8, device=DEV)
    u_units = flat_u[3:].view(nseries + 1, out_stride)
    engine.merge_batch_units_dev(d_ts, d_vals, d_units, d_counts, R,
                                 u_ts[:nseries], u_vals[:nseries],
                                 u_units[:nseries], u_counts, u_errs)
    p_ts, p_vals, p_counts, p_errs = outputs()
    engine.merge_batch_dev(d_ts, d_vals, d_counts, R, p_ts[:nseries],
                           p_vals[:nseries], p_counts, p_errs)
    torch.cuda.synchronize()

    # the plain merge's outputs, byte for byte, guard rows included
    assert np.array_equal(u_ts.cpu().numpy(), p_ts.cpu().numpy())
    assert np.array_equal(u_vals.view(torch.int64).cpu().numpy(),
                          p_vals.view(torch.int64).cpu().numpy())
    assert np.array_equal(u_counts.cpu().numpy(), p_counts.cpu().numpy())
    assert np.array_equal(u_errs.cpu().numpy(), p_errs.cpu().numpy())
    assert np.all(u_errs.cpu().numpy() == 0)

    g_ts = u_ts.cpu().numpy()
    g_vals = u_vals.cpu().numpy()
    g_counts = u_counts.cpu().numpy()
    h_flat = flat_u.cpu().numpy()
    g_units = h_flat[3:].reshape(nseries + 1, out_stride)
    assert np.all(h_flat[:3] == USENT)
    for i, (m_ts, m_vals, m_units) in enumerate(model):
        n = len(m_ts)
        assert g_counts[i] == n, i
        assert g_ts[i, :n].tolist() == m_ts, i
        assert g_vals[i, :n].tolist() == m_vals, i
        assert g_units[i, :n].tolist() == m_units, i
        assert np.all(g_ts[i, n:] == SENTINEL), i
        assert np.all(g_units[i, n:] == USENT), i
    assert np.all(g_ts[nseries] == SENTINEL)
    assert np.all(g_units[nseries] == USENT)


def test_capacity_keeps_the_units_of_the_stored_points(torch, engine):
    """out_stride below a merged count: CAPACITY, and units for exactly the
    points that were stored."""
    R = 2
    ts, vals, units, counts = cases.merge_inputs(R)
    _, nseries, stride = ts.shape
    model = cases.merge_model(ts, vals, units, counts)
    out_stride = 5
    assert any(len(m[0]) > out_stride for m in model)
    d = lambda a, w: torch.from_numpy(a.reshape(R * nseries, w)).to(DEV)
    o_ts = torch.full((nseries, out_stride), SENTINEL, dtype=torch.int64,
                      device=DEV)
    o_vals = torch.zeros((nseries, out_stride), dtype=torch.float64,
                         device=DEV)
    o_units = torch.full((nseries + 1, out_stride), USENT, dtype=torch.uint8,
                         device=DEV)
    o_counts = torch.full((nseries,), -1, dtype=torch.int32, device=DEV)
    o_errs = torch.full((nseries,), -1, dtype=torch.int32, device=DEV)
    engine.merge_batch_units_dev(
        d(ts, stride), d(vals, stride), d(units, stride),
        torch.from_numpy(counts.reshape(-1).astype(np.int32)).to(DEV), R,
        o_ts, o_vals, o_units[:nseries], o_counts, o_errs)
    torch.cuda.synchronize()
    g_units = o_units.cpu().numpy()
    g_counts, g_errs = o_counts.cpu().numpy(), o_errs.cpu().numpy()
    for i, (m_ts, _, m_units) in enumerate(model):
        n = min(len(m_ts), out_stride)
        assert g_counts[i] == n, i
        assert g_errs[i] == (6 if len(m_ts) > out_stride else 0), i
        assert g_units[i, :n].tolist() == m_units[:n], i
        assert np.all(g_units[i, n:] == USENT), i
    assert np.all(g_units[nseries] == USENT)

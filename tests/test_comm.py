"""The y-slab communicator INSIDE the C library (breeze.jl_amd/csrc/bz_comm.hip; BASELINE.json north_star: "RCCL halo exchange and FFT
all-to-all" behind the C ABI).  One MI355X is available to the tests, so
  * the whole distributed step (bz_time_step_anelastic on slab contexts: halo exchange overlapped with the interior tendency tiles,
    transposes, phi row) runs with 1, 2 and 4 ranks as host threads sharing cuda:0 over the library's in-process transport and is
    compared DIRECTLY WITH THE ORACLE on the whole domain (and, bit for bit where the arithmetic is the same, with the single-GPU seam);
  * the RCCL transport runs with one rank (ncclCommInitRank(1, id, 0), self send / recv groups): the dlopen, the communicator
    bootstrap from the 128-byte id and every ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd call site execute for real.
What only an 8-GPU node can show — messages crossing xGMI — is left to the round-end scaling run."""
import os
import sys
import threading
import uuid

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTENT = ((-10e3, 10e3), (-10e3, 10e3), (0.0, 10e3))
pytestmark = pytest.mark.gpu


def theta_ic(x, y, z):
    r = np.sqrt(x ** 2 + (y - 1500.0) ** 2 + (z - 3000.0) ** 2)
    return 300.0 * np.exp(1e-6 * z / 9.81) + 10.0 * np.maximum(0.0, 1.0 - r / 2.5e3)


def q_ic(x, y, z):
    return 6e-3 * np.exp(-z / 2500.0) * (1.0 + 0.3 * np.sin(2 * np.pi * y / 20e3)) + 0 * x


def run_slabs(bz, size, world, steps, dt, moist, transport=None):
    import torch
    from breeze_jl_amd import distributed as bz_dist
    G = bz.RectilinearGrid(size, x=EXTENT[0], y=EXTENT[1], z=EXTENT[2])
    group = transport or ("local:" + uuid.uuid4().hex)
    models, errors = [None] * world, []
    kw = dict(θ=theta_ic, u=3.0, v=-2.0)
    if moist:
        kw["qᵗ"] = q_ic

    def run(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):          # one HIP stream per rank, as one process per GPU would have
                m = bz_dist.SlabAtmosphereModel(G, rank, world, advection=bz.WENO(), potential_temperature=300, device="cuda:0",
                                                transport=group)
                m.set(**kw)
                for _ in range(steps):
                    m.time_step(dt)
                m.synchronize()
            models[rank] = m
        except Exception as e:      # noqa: BLE001
            import traceback
            errors.append((rank, repr(e), traceback.format_exc()))

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    return models


FIELDS = {"ru": lambda m: m.momentum["ρu"], "rv": lambda m: m.momentum["ρv"], "rw": lambda m: m.momentum["ρw"],
          "rtheta": lambda m: m.potential_temperature_density, "rq": lambda m: m.moisture_density, "T": lambda m: m.temperature,
          "u": lambda m: m.velocities["u"], "theta": lambda m: m.potential_temperature}


def test_local_transport_self_messages(bz, oracle, monkeypatch):
    """The same single-rank self-addressed step over the in-process transport (the message path of the multi-rank runs below)."""
    monkeypatch.setenv("BZ_COMM_SELF_MESSAGES", "1")
    models = run_slabs(bz, (32, 16, 16), 1, 1, 2.0, False)
    assert models[0].comm_info()[1] > 0


@pytest.mark.parametrize("world,size,moist", [(1, (32, 24, 16), False), (2, (32, 24, 16), True), (4, (32, 48, 16), False), (2, (70, 32, 12), True),
                                              # shapes the hand-written x transforms take on slab ranks (Nx a power of two, 8 | local Ny): messages of
                                              # the all-to-alls written / read in place, zero padding of the last wavenumber block
                                              (2, (64, 32, 16), True), (4, (32, 64, 12), False), (2, (16, 16, 8), False),
                                              (2, (1024, 16, 6), False),       # BASELINE configs[3] row length: teams of two wavefronts
                                              # round 6: EIGHT ranks — the target node's world size.  33 half-spectrum planes over
                                              # 8 ranks (5 5 5 5 5 5 3 0 after the split by whole blocks: an uneven and an empty share) with 8-row
                                              # slabs, moist; 64-row slabs of 512-cell rows (the strong 512^3 split's slab: four 16-row tiles of the
                                              # y-momentum kernel, the outer two waiting for halo rows); 17 planes over 8 ranks
                                              (8, (64, 64, 16), True), (8, (512, 512, 6), False), (8, (32, 48, 10), True)])
def test_library_owned_slab_step_matches_the_oracle(bz, oracle, world, size, moist):
    steps, dt = 2, 2.0
    models = run_slabs(bz, size, world, steps, dt, moist)
    og = oracle.Grid(size, x=EXTENT[0], y=EXTENT[1], z=EXTENT[2])
    om = oracle.OracleModel(og, potential_temperature=300.0)
    kw = dict(theta=theta_ic, u=3.0, v=-2.0)
    if moist:
        kw["qt"] = q_ic
    om.set(**kw)
    for _ in range(steps):
        om.time_step(dt)
    mom = max(np.abs(og.interior(getattr(om, n), zface=(n == "rw"))).max() for n in ("ru", "rv", "rw"))      # a vector's components share its scale
    for name, get in FIELDS.items():
        got = np.concatenate([get(m).interior_cpu() for m in models], axis=1)
        want = og.interior(getattr(om, name), zface=(name == "rw"))
        scale = mom if name in ("ru", "rv", "rw") else max(np.max(np.abs(want)), 1e-3)
        err = np.max(np.abs(got - want)) / scale
        # 1024 x 16 x 6 on the 20 km box is a 64 : 1 anisotropic grid: the single-GPU step (hand-written or library transforms alike)
        # differs from the oracle by 1.0e-9 there, and the slab step equals the single-GPU step to 1e-14
        assert err < (5e-9 if size[0] == 1024 else 1e-9), (name, err)
    name, nbytes, nex = models[0].comm_info()
    assert name == "local" and (nbytes > 0) == (world > 1) and nex > 0 if world > 1 else True


def test_library_owned_slab_step_equals_the_single_gpu_seam(bz, monkeypatch):
    """Two and four ranks against the single-GPU lean seam on the same domain: same kernels, same arithmetic per cell except the
    Poisson solve (1-D batched plans + transposes instead of the 2-D plan): 1e-11 of the field scale; and every y halo row the next
    operator could read is what the periodic single-GPU field holds there."""
    size, steps, dt = (32, 32, 16), 2, 2.0
    G = bz.RectilinearGrid(size, x=EXTENT[0], y=EXTENT[1], z=EXTENT[2])
    ref = bz.AtmosphereModel(G, dynamics=bz.AnelasticDynamics(bz.ReferenceState(G, potential_temperature=300)), advection=bz.WENO())
    ref.set(θ=theta_ic, u=3.0, v=-2.0, qᵗ=q_ic)
    for _ in range(steps):
        ref.time_step(dt)
    ref.synchronize()
    for world in (2, 4):
        models = run_slabs(bz, size, world, steps, dt, True)
        Ny = size[1] // world
        for name, get in FIELDS.items():
            want_parent = get(ref).cpu()
            scale = max(np.max(np.abs(want_parent)), 1e-3)
            for r, m in enumerate(models):
                got = get(m).cpu()                                   # (z, Ny + 2 Hy, x) parent of the slab, y halos included
                rows = [(r * Ny - 3 + j) % size[1] + 3 for j in range(Ny + 6)]       # parent rows of the periodic single-GPU field
                zs = slice(3, 3 + size[2] + (1 if name == "rw" else 0))
                ys = slice(3, -3) if name == "T" else slice(None)     # T is only ever read in the own column: its y halos do not travel
                err = np.max(np.abs(got[zs, ys, 3:-3] - want_parent[zs][:, rows][:, ys, 3:-3])) / scale
                assert err < 1e-11, (world, name, r, err)


def test_overlap_and_blocking_exchanges_agree_bitwise(bz, monkeypatch):
    """BZ_COMM_NO_OVERLAP=1 runs the closing halo exchange of a stage on the main stream before any tendency tile; the default runs
    it on the side stream under the interior tiles.  Same arithmetic, so the same bits."""
    size = (32, 48, 16)
    a = run_slabs(bz, size, 2, 2, 2.0, True)
    monkeypatch.setenv("BZ_COMM_NO_OVERLAP", "1")
    b = run_slabs(bz, size, 2, 2, 2.0, True)
    for name, get in FIELDS.items():
        for ma, mb in zip(a, b):
            assert np.array_equal(get(ma).cpu(), get(mb).cpu()), name


@pytest.mark.parametrize("self_messages", [False, True])
def test_rccl_transport_with_one_rank(bz, oracle, self_messages, monkeypatch):
    """ncclCommInitRank on a communicator of one rank (dlopen, unique id, communicator bootstrap) and two full steps on it.  With
    BZ_COMM_SELF_MESSAGES=1 the single rank addresses every message of the step to itself THROUGH RCCL — the halo rows (two sends and
    two receives per group, the ordering of the two-rank case), the all-to-all blocks of both transposes, the phi row — so each
    ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd call site of the library runs on the real transport, side stream included."""
    if self_messages:
        monkeypatch.setenv("BZ_COMM_SELF_MESSAGES", "1")
    models = run_slabs(bz, (32, 16, 16), 1, 2, 2.0, False, transport="rccl")
    if self_messages:
        assert models[0].comm_info()[1] > 0
    assert models[0].comm_info()[0] == "rccl"
    og = oracle.Grid((32, 16, 16), x=EXTENT[0], y=EXTENT[1], z=EXTENT[2])
    om = oracle.OracleModel(og, potential_temperature=300.0)
    om.set(theta=theta_ic, u=3.0, v=-2.0)
    for _ in range(2):
        om.time_step(2.0)
    got = models[0].momentum["ρw"].interior_cpu()
    want = og.interior(om.rw, zface=True)
    assert np.max(np.abs(got - want)) / np.max(np.abs(want)) < 1e-9


@pytest.mark.parametrize("world,order,size", [pytest.param(1, 5, (32, 32, 16), id="1-5"), pytest.param(2, 5, (32, 32, 16), id="2-5"),
                                              pytest.param(4, 5, (32, 32, 16), id="4-5"), pytest.param(2, 9, (32, 32, 16), id="2-9"),
                                              # rows of whole 64-cell tiles: local Ny = 32, 16, 8 rows are 4, 2, 1 tile rows, so every rank
                                              # runs the z-marching closure kernels and their y-slab branch (below)
                                              pytest.param(1, 5, (64, 32, 16), id="1-5-64x32x16"), pytest.param(2, 5, (64, 32, 16), id="2-5-64x32x16"),
                                              pytest.param(4, 5, (64, 32, 16), id="4-5-64x32x16")])
def test_bomex_physics_on_library_slabs_matches_the_oracle(bz, oracle, world, order, size, monkeypatch):
    """The physics list of BASELINE configs[2] — WENO5 + saturation adjustment + SmagorinskyLilly + Coriolis / geostrophic /
    subsidence / profile forcings + bottom fluxes — decomposed into y-slabs with the library-owned communicator (fused-RK tier with
    halo exchanges, horizontal averages all-reduced over the ranks, viscosity kernel covering the rows next to the slab), against
    the single-process oracle: 2e-9 of the field scale after three steps, the tolerance of the single-GPU test of the same physics
    (tests/test_closure.py::test_bomex_stack_time_steps_match_oracle).

    64 x 32 x 16: the slab branch of the z-marching closure kernels (csrc/bz_closure.hip: bz_compute_closure_fields, `if (ctx->slab_mode)`):
    k_smagorinsky_march covers the slab's own rows and two one-row launches of the cell-per-thread kernel the rows -1 and Ny, which
    k_closure_march reads unwrapped.  With four ranks a slab is a single tile row whose two outer rows both come from the neighbours.  Every
    rank reports the march (closure_marches()); the prognostic fields, and nu_e on rows -1 .. Ny of every rank, carry the bits of the same run
    with BZ_NO_CLOSURE_MARCH=1, whose one cell-per-thread launch covers the Ny + 2 rows with the same expressions.  (A profile record is one
    per bracketed group, however many kernels it covers, so the profile counts one `smagorinsky_viscosity` per evaluation in both runs: the
    rows themselves are the evidence that the edge launches ran — a row never written keeps the zeros of its allocation.)"""
    import sys
    import os
    import torch
    sys.path.insert(0, os.path.dirname(__file__))
    from breeze_jl_amd import distributed as bz_dist
    from oracle.closure import SmagorinskyLilly
    from test_closure import _turbulent_ic
    from test_forcings import EXTENT as FEXT, _hip_forcing_kwargs, _oracle_forcings
    halo = (3, 3, 3) if order == 5 else (5, 5, 5)      # order 9 (examples/bomex.jl:204): the operator-by-operator distributed step
    og = oracle.Grid(size, x=FEXT[0], y=FEXT[1], z=FEXT[2], halo=halo)
    om = oracle.OracleModel(og, surface_pressure=101500.0, potential_temperature=299.1, microphysics="SaturationAdjustment",
                            closure=SmagorinskyLilly(), forcings=_oracle_forcings(oracle, og), advection=f"WENO{order}")
    ic = _turbulent_ic(om, 5)
    om.set(**ic)
    for _ in range(3):
        om.time_step(3.0)
    G = bz.RectilinearGrid(size, x=FEXT[0], y=FEXT[1], z=FEXT[2], halo=halo)
    Ny = size[1] // world

    def run_ranks():
        group = "local:" + uuid.uuid4().hex
        models, errors = [None] * world, []

        def run(rank):
            try:
                torch.cuda.set_device(0)
                with torch.cuda.stream(torch.cuda.Stream()):
                    m = bz_dist.LibrarySlabAtmosphereModel(G, rank, world, transport=group, surface_pressure=101500.0,
                                                           potential_temperature=299.1, advection=bz.WENO(order=order), device="cuda:0",
                                                           closure=bz.SmagorinskyLilly(),
                                                           microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()),
                                                           **_hip_forcing_kwargs(bz))
                    sl = slice(rank * Ny, (rank + 1) * Ny)
                    m.set(θ=ic["theta"][:, sl, :], qᵗ=ic["qt"][:, sl, :], u=ic["u"][:, sl, :], v=ic["v"][:, sl, :])
                    for _ in range(3):
                        m.time_step(3.0)
                    m.synchronize()
                models[rank] = m
            except Exception as e:      # noqa: BLE001
                import traceback
                errors.append((rank, repr(e), traceback.format_exc()))

        threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        return models

    monkeypatch.delenv("BZ_NO_CLOSURE_MARCH", raising=False)
    models = run_ranks()
    mom = max(np.abs(og.interior(getattr(om, n), zface=(n == "rw"))).max() for n in ("ru", "rv", "rw"))
    for name in ("ru", "rv", "rw", "rtheta", "rq", "T"):
        got = np.concatenate([FIELDS[name](m).interior_cpu() for m in models], axis=1)
        want = og.interior(getattr(om, name), zface=(name == "rw"))
        scale = mom if name in ("ru", "rv", "rw") else np.abs(want).max()
        assert np.abs(got - want).max() / scale < (2e-9 if order == 5 else 2e-8), (name, np.abs(got - want).max() / scale)
    ql = np.concatenate([m.microphysical_fields["qˡ"].interior_cpu() for m in models], axis=1)
    assert np.abs(ql - og.interior(om.ql)).max() < 1e-9
    assert [m.closure_marches() for m in models] == [size[0] % 64 == 0] * world
    if size[0] % 64:
        return
    monkeypatch.setenv("BZ_NO_CLOSURE_MARCH", "1")          # read when a context is created
    try:
        plain = run_ranks()
    finally:
        monkeypatch.delenv("BZ_NO_CLOSURE_MARCH", raising=False)
    assert not any(m.closure_marches() for m in plain)
    for name in ("ru", "rv", "rw", "rtheta", "rq"):
        got = np.concatenate([FIELDS[name](m).interior_cpu() for m in models], axis=1)
        assert np.array_equal(got, np.concatenate([FIELDS[name](m).interior_cpu() for m in plain], axis=1)), name
    H = halo[0]
    for r, (m, p) in enumerate(zip(models, plain)):
        rows = slice(H - 1, H + Ny + 1)                         # rows -1 .. Ny of the slab
        nu, nu_plain = (x.closure_fields["νₑ"].cpu()[H:H + size[2], rows, H:H + size[0]] for x in (m, p))
        assert np.array_equal(nu, nu_plain), r
        assert nu[:, 0].max() > 0 and nu[:, -1].max() > 0, r     # the rows beyond the slab were written


@pytest.mark.parametrize("world", [1, 2])
def test_tracers_on_library_slabs_match_the_oracle(bz, oracle, world):
    """User tracers (`tracers = (:a, :b)`, test/tracer_dynamics.jl) on y-slabs: the tracer tendencies and RK updates ride beside the
    fused kernels of the library's distributed step and the specific fields join the per-stage halo exchange.  Tracer b varies in
    y across the slab edge, so a missing exchange shows at the first stage."""
    import torch
    from breeze_jl_amd import distributed as bz_dist
    from helpers import bubble_theta
    size, ext = (32, 24, 16), dict(x=(-4e3, 4e3), y=(-3e3, 3e3), z=(0.0, 8e3))
    og = oracle.Grid(size, **ext)
    om = oracle.OracleModel(og, potential_temperature=300.0, tracers=2)
    th = bubble_theta(300.0, 9.81, r0=2e3, zc=2500.0)
    a = lambda x, y, z: np.sin(2 * np.pi * x / 8e3) * np.exp(-z / 4e3) + 0 * y
    b = lambda x, y, z: 1.0 + 0.5 * np.cos(2 * np.pi * y / 6e3) * (z / 8e3) + 0 * x
    om.set(theta=th, u=3.0, v=-2.0, rc0=a, rc1=b)
    ic = {n: og.interior(getattr(om, n)).copy() for n in ("rc0", "rc1", "theta")}
    for _ in range(3):
        om.time_step(2.0)
    G = bz.RectilinearGrid(size, **ext)
    group = "local:" + uuid.uuid4().hex
    Ny = size[1] // world
    models, errors = [None] * world, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                m = bz_dist.LibrarySlabAtmosphereModel(G, rank, world, transport=group, potential_temperature=300.0,
                                                       advection=bz.WENO(order=5), device="cuda:0", tracers=("a", "b"))
                sl = slice(rank * Ny, (rank + 1) * Ny)
                m.tracers["a"].set_interior(ic["rc0"][:, sl, :])
                m.tracers["b"].set_interior(ic["rc1"][:, sl, :])
                m.set(θ=ic["theta"][:, sl, :], u=3.0, v=-2.0)
                for _ in range(3):
                    m.time_step(2.0)
                m.synchronize()
            models[rank] = m
        except Exception as e:      # noqa: BLE001
            import traceback
            errors.append((rank, repr(e), traceback.format_exc()))

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for n, k in (("rc0", "a"), ("rc1", "b")):
        want = og.interior(getattr(om, n))
        got = np.concatenate([m.tracers[k].interior_cpu() for m in models], axis=1)
        assert np.abs(got - want).max() < 1e-9 * np.abs(want).max(), n
        want_c = og.interior(getattr(om, "c" + n[2:]))
        got_c = np.concatenate([m.specific_tracers[k].interior_cpu() for m in models], axis=1)
        assert np.abs(got_c - want_c).max() < 1e-9 * np.abs(want_c).max()
    want = og.interior(om.rtheta)
    got = np.concatenate([m.potential_temperature_density.interior_cpu() for m in models], axis=1)
    assert np.abs(got - want).max() < 1e-10 * np.abs(want).max()


def _library_slabs(bz, G, world, make_kwargs, setter, steps, dt):
    import torch
    from breeze_jl_amd import distributed as bz_dist
    group = "local:" + uuid.uuid4().hex
    models, errors = [None] * world, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                m = bz_dist.LibrarySlabAtmosphereModel(G, rank, world, transport=group, device="cuda:0", **make_kwargs())
                Ny = G.Ny // world
                setter(m, slice(rank * Ny, (rank + 1) * Ny))
                for _ in range(steps):
                    m.time_step(dt)
                m.synchronize()
            models[rank] = m
        except Exception as e:      # noqa: BLE001
            import traceback
            errors.append((rank, repr(e), traceback.format_exc()))

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    return models


@pytest.mark.parametrize("case", ["weno9", "static_energy", "kessler", "mixed_orders_sponge_heating"])
def test_operator_by_operator_slab_step_matches_the_oracle(bz, oracle, case):
    """Model options outside the fused tiers take the operator-by-operator distributed step (bz_comm.hip: dist_time_step_operators — the
    reference's call order with the library's exchanges in place of the local halo fills): WENO(order = 9), formulation = :StaticEnergy
    and DCMIP2016 Kessler species on the anelastic core, two ranks, against the single-process oracle."""
    world, steps = 2, 2
    if case == "kessler":
        size, ext, dt = (16, 16, 20), ((0.0, 4e3), (0.0, 4e3), (0.0, 5e3)), 5.0
        og = oracle.Grid(size, x=ext[0], y=ext[1], z=ext[2])
        om = oracle.OracleModel(og, surface_pressure=1e5, potential_temperature=300.0, microphysics="Kessler")
        G = bz.RectilinearGrid(size, x=ext[0], y=ext[1], z=ext[2])
        tc = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
        mk = lambda: dict(surface_pressure=1e5, potential_temperature=300.0, advection=bz.WENO(order=5), thermodynamic_constants=tc,
                          microphysics=bz.DCMIP2016KesslerMicrophysics())
        bub = lambda x, y, z: np.maximum(0.0, 1.0 - np.sqrt((x - 2e3) ** 2 + (y - 2e3) ** 2 + (z - 1500.0) ** 2) / 1200.0)
        ic = dict(qt=lambda x, y, z: 0.016 * np.exp(-z / 3000.0) + 0.004 * bub(x, y, z), theta=lambda x, y, z: 300.0 + 0.004 * z + 1.0 * bub(x, y, z),
                  qcl=lambda x, y, z: 0.003 * bub(x, y, z), qr=lambda x, y, z: 0.001 * bub(x, y, z), u=2.0, v=-1.0)
        om.set(**ic)
        x, y, z = og.nodes("ccc")
        full = {k: (np.broadcast_to(v(x, y, z), (size[2], size[1], size[0])).copy() if callable(v) else v) for k, v in ic.items()}
        setter = lambda m, sl: m.set(qᵗ=full["qt"][:, sl, :], θ=full["theta"][:, sl, :], qcl=full["qcl"][:, sl, :], qr=full["qr"][:, sl, :], u=2.0, v=-1.0)
        names, tol = ("ru", "rv", "rw", "rtheta", "rq", "T"), 1e-8
    else:
        order = 9 if case in ("weno9", "mixed_orders_sponge_heating") else 5
        size, dt = (32, 24, 16), 2.0
        halo = (5, 5, 5) if order == 9 else (3, 3, 3)
        og = oracle.Grid(size, x=EXTENT[0], y=EXTENT[1], z=EXTENT[2], halo=halo)
        form = "StaticEnergy" if case == "static_energy" else "LiquidIcePotentialTemperature"
        G = bz.RectilinearGrid(size, x=EXTENT[0], y=EXTENT[1], z=EXTENT[2], halo=halo)
        if case == "mixed_orders_sponge_heating":
            # round-3 options on slabs: momentum WENO9 + scalars WENO5, a Gaussian sponge on rho w, a 3-D heating keyed theta — all
            # cell-local additions to the operator-by-operator distributed step
            ztop = EXTENT[2][1]
            gauss = lambda z: np.exp(-(z - ztop) ** 2 / (2 * (0.2 * ztop) ** 2))
            heat = lambda x, y, z: 2e-3 * np.exp(-((x - 0.2 * EXTENT[0][1]) ** 2 + (y - 0.1 * EXTENT[1][1]) ** 2) / (0.3 * EXTENT[0][1]) ** 2) + 0 * z
            om = oracle.OracleModel(og, potential_temperature=300.0, advection="WENO9", scalar_advection="WENO5")
            om.relaxation = {"rw": (0.05 * gauss(og.zf), np.zeros(og.Nz + 1))}
            xx, yy, zz = og.nodes("ccc")
            om.field_forcing = (np.broadcast_to(heat(xx, yy, zz), (size[2], size[1], size[0])).copy(), True)
            mk = lambda: dict(potential_temperature=300.0, momentum_advection=bz.WENO(order=9), scalar_advection=bz.WENO(order=5),
                              forcing={"ρw": bz.Relaxation(rate=0.05, mask=gauss), "θ": bz.Forcing(heat)})
        else:
            om = oracle.OracleModel(og, potential_temperature=300.0, advection=f"WENO{order}", formulation=form)
            mk = lambda: dict(potential_temperature=300.0, advection=bz.WENO(order=order), formulation=form)
        om.set(theta=theta_ic, u=3.0, v=-2.0)
        x, y, z = og.nodes("ccc")
        th = np.broadcast_to(theta_ic(x, y, z), (size[2], size[1], size[0])).copy()
        setter = lambda m, sl: m.set(θ=th[:, sl, :], u=3.0, v=-2.0)
        names, tol = ("ru", "rv", "rw", "rtheta", "T"), (2e-8 if order == 9 else 1e-9)
    for _ in range(steps):
        om.time_step(dt)
    models = _library_slabs(bz, G, world, mk, setter, steps, dt)
    get = dict(FIELDS)
    get["rtheta"] = lambda m: (m.energy_density if case == "static_energy" else m.potential_temperature_density)
    mom = max(np.abs(og.interior(getattr(om, n), zface=(n == "rw"))).max() for n in ("ru", "rv", "rw"))
    for name in names:
        got = np.concatenate([get[name](m).interior_cpu() for m in models], axis=1)
        want = og.interior(getattr(om, name), zface=(name == "rw"))
        scale = mom if name in ("ru", "rv", "rw") else max(np.max(np.abs(want)), 1e-3)
        assert np.max(np.abs(got - want)) / scale < tol, (case, name, np.max(np.abs(got - want)) / scale)


def test_stale_diagnostics_on_a_slab_model_need_an_explicit_collective_refresh(bz):
    """rebuilding the diagnostics of a slab model exchanges halos — a collective.  After time_steps(..., diagnose_last=False) a
    field read no longer enters it on its own (a rank-0-only log line would wait for ranks that never come): it raises, naming
    model.refresh_diagnostics(), which every rank calls; afterwards the fields read what a diagnosed call leaves."""
    import torch
    from breeze_jl_amd import distributed as bz_dist
    G = bz.RectilinearGrid((32, 16, 12), x=EXTENT[0], y=EXTENT[1], z=EXTENT[2])

    def make():
        m = bz_dist.LibrarySlabAtmosphereModel(G, 0, 1, transport="local:" + uuid.uuid4().hex, device="cuda:0", potential_temperature=300.0,
                                               advection=bz.WENO())
        m.set(θ=theta_ic, u=3.0, v=-2.0, qᵗ=q_ic)
        return m

    a, b = make(), make()
    a.time_steps(2.0, 2, diagnose_last=True)
    b.time_steps(2.0, 2, diagnose_last=False)
    b.synchronize()
    with pytest.raises(RuntimeError, match="refresh_diagnostics"):
        b.temperature.interior_cpu()
    assert np.array_equal(b.potential_temperature_density.interior_cpu(), a.potential_temperature_density.interior_cpu())      # prognostic reads are fine
    b.refresh_diagnostics()
    for get in (lambda m: m.temperature, lambda m: m.velocities["u"], lambda m: m.potential_temperature):
        assert np.array_equal(get(b).interior_cpu(), get(a).interior_cpu())

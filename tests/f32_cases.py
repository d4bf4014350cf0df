"""Float32 step cases, shared by the GPU tests that run them on the device against the Float64 oracle (tests/test_float32.py,
tests/test_float32_increments.py, tests/test_gpu_compressible.py) and by the CPU test that keeps their tolerances honest
(tests/test_float32_tolerances.py): one builder per set-up, so the two cannot drift apart.

A case builds the oracle model (and, given `bz`, the device model) with its initial state set; `defect` changes the oracle alone:
    {"dt": 1.01}       every step 1 % too long (the runner applies it)
    {"weno": True}     the neighbouring WENO order (7 for 5, 9 for 7, 7 for 9), halo widened where needed
    {"substeps": 5}    five acoustic substeps where the case asks for six (compressible cases)."""
import numpy as np

EXT = ((-10e3, 10e3), (-10e3, 10e3), (0.0, 10e3))

# device getters of the oracle's field names
ANELASTIC_GET = {
    "ru": lambda m: m.momentum["ρu"], "rv": lambda m: m.momentum["ρv"], "rw": lambda m: m.momentum["ρw"],
    "rtheta": lambda m: m.potential_temperature_density, "rq": lambda m: m.moisture_density, "T": lambda m: m.temperature,
    "rc0": lambda m: m.tracers["a"], "rqcl": lambda m: m.microphysical_fields["ρqᶜˡ"], "rqr": lambda m: m.microphysical_fields["ρqʳ"],
}
COMPRESSIBLE_GET = {
    "rho_d": lambda m: m.dynamics.dry_density, "rtheta": lambda m: m.potential_temperature_density, "rq": lambda m: m.moisture_density,
    "T": lambda m: m.temperature, "p": lambda m: m.dynamics.pressure,
    "ru": lambda m: m.momentum["ρu"], "rv": lambda m: m.momentum["ρv"], "rw": lambda m: m.momentum["ρw"],
}


def oracle_fields(om, names):
    g = om.grid
    return {n: np.array(g.interior(getattr(om, n), n == "rw"), dtype=np.float64) for n in names}


def device_fields(hm, names, compressible=False):
    get = COMPRESSIBLE_GET if compressible else ANELASTIC_GET
    return {n: get[n](hm).interior_cpu().astype(np.float64) for n in names}


def _weno(order, d):
    """(oracle advection name, minimum halo) of a case of WENO `order` under defect `d`."""
    if d.get("weno"):
        order = {5: 7, 7: 9, 9: 7}[order]
    return f"WENO{order}", (order + 1) // 2


def _halo(ndim, base, need):
    h = max(base, need)
    return (h,) * ndim


def moist_q(x, y, z):
    """The vapour profile of the moist lean-seam cases (tests/test_gpu_parity.py: _moist_q)."""
    r = np.sqrt(x ** 2 + (y - 1000.0) ** 2 + (z - 2500.0) ** 2)
    return 8e-3 * np.exp(-z / 2500.0) * (1.0 + 0.3 * np.maximum(0.0, 1.0 - r / 3e3))


def stretched_faces(Nz, Lz=10e3):
    k = np.arange(Nz + 1) / Nz
    return Lz * (0.6 * k + 0.4 * k ** 2)


class Case:
    """A Float32 set-up: `build(orc, oc, bz, defect)` -> (oracle model, device model or None), both with their initial state set.
    kind: the F32_INCREMENT_TOL table; fields: the oracle names compared; dt, steps: what the tests run; env: device switches."""

    def __init__(self, name, kind, fields, dt, steps, build, defects=("dt",), env=None, key=None):
        self.name, self.kind, self.fields, self.dt, self.steps, self._build = name, kind, tuple(fields), dt, steps, build
        self.defects, self.env = tuple(defects), dict(env or {})
        self.key = key or name      # cases that differ in device switches only share the oracle set-up (and its key)

    def build(self, orc, oc, bz=None, defect=None):
        return self._build(orc, oc, bz, dict(defect or {}))

    def __repr__(self):
        return self.name


def run_oracle(case, orc, oc, defect=None, at=None):
    """(start, {step: fields}) of the oracle run of `case` (with `defect`), fields read after each step listed in `at`."""
    d = dict(defect or {})
    om, _ = case.build(orc, oc, None, d)
    start = oracle_fields(om, case.fields)
    at = tuple(at or (case.steps,))
    out = {}
    for s in range(1, max(at) + 1):
        om.time_step(case.dt * d.get("dt", 1.0))
        if s in at:
            out[s] = oracle_fields(om, case.fields)
    return start, out


# ---- anelastic bubble: tests/test_float32.py time steps and the lean-seam sweep --------------------------------------------------------------
def bubble(size, moist=False, topology=("Periodic", "Periodic", "Bounded"), stretched=False, forcings=False, dtheta=10.0,
           u=3.0, v=-2.0, seam=0.0):
    from helpers import bubble_theta
    from test_forcings import F0, ug_profile, vg_profile

    def build(orc, oc, bz, d):
        adv, need = _weno(5, d)
        z = stretched_faces(size[2]) if stretched else EXT[2]
        og = orc.Grid(size, x=EXT[0], y=EXT[1], z=z, topology=topology, halo=_halo(3, 3, need))
        okw = {}
        if forcings:
            from oracle.forcings import ColumnForcings
            col = lambda f: np.array([f(v) for v in og.zc])
            okw["forcings"] = ColumnForcings(Fu=-F0 * col(vg_profile), Fv=F0 * col(ug_profile), coriolis_f=F0)
        om = orc.OracleModel(og, potential_temperature=300.0, advection=adv, **okw)
        bub = bubble_theta(300.0, 9.81, dtheta=dtheta)
        # seam: a second bubble of that amplitude centred on the periodic x seam, so that the cells on either side of it differ
        seam_r = lambda x, y, z: np.sqrt(np.minimum(np.abs(x - EXT[0][0]), np.abs(x - EXT[0][1])) ** 2 + y ** 2 + (z - 3000.0) ** 2)
        th = bub if not seam else (lambda x, y, z: bub(x, y, z) + seam * np.maximum(0.0, 1.0 - seam_r(x, y, z) / 2e3))
        ic = dict(theta=th, u=u, v=v)
        if moist:
            ic["qt"] = moist_q
        om.set(**ic)
        hm = None
        if bz is not None:
            T = getattr(bz, topology[1])
            grid = bz.RectilinearGrid(size, x=EXT[0], y=EXT[1], z=z, topology=(bz.Periodic, T, bz.Bounded), float_type=np.float32)
            hkw = {}
            if forcings:
                geo = bz.geostrophic_forcings(ug_profile, vg_profile)
                hkw = dict(coriolis=bz.FPlane(f=F0), forcing={"u": geo.u, "v": geo.v})
            hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)),
                                    advection=bz.WENO(), **hkw)
            hm.set(θ=th, u=u, v=v, **({"qᵗ": moist_q} if moist else {}))
        return om, hm
    return build


def bubble_case(name, size, moist=False, steps=3, dt=2.0, env=None, **kw):
    fields = ("ru", "rv", "rw", "rtheta", "T") + (("rq",) if moist else ())
    return Case(name, "anelastic", fields, dt, steps, bubble(size, moist=moist, **kw), defects=("dt", "weno"), env=env,
                key=repr(("bubble", tuple(size), moist, steps, dt, sorted(kw.items()))))


# ---- tests/test_float32.py: the remaining step tests --------------------------------------------------------------------------------------------
def _bomex(orc, oc, bz, d):
    from oracle.closure import SmagorinskyLilly
    from test_closure import _turbulent_ic
    from test_forcings import EXTENT, _hip_forcing_kwargs, _oracle_forcings
    adv, need = _weno(5, d)
    size = (32, 24, 16)
    og = orc.Grid(size, x=EXTENT[0], y=EXTENT[1], z=EXTENT[2], halo=_halo(3, 3, need))
    om = orc.OracleModel(og, surface_pressure=101500.0, potential_temperature=299.1, microphysics="SaturationAdjustment",
                         closure=SmagorinskyLilly(), forcings=_oracle_forcings(orc, og), advection=adv)
    ic = _turbulent_ic(om, 5)
    om.set(**ic)
    hm = None
    if bz is not None:
        grid = bz.RectilinearGrid(size, x=EXTENT[0], y=EXTENT[1], z=EXTENT[2], float_type=np.float32)
        ref = bz.ReferenceState(grid, surface_pressure=101500.0, potential_temperature=299.1)
        hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), closure=bz.SmagorinskyLilly(),
                                microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()), **_hip_forcing_kwargs(bz))
        hm.set(θ=ic["theta"], qᵗ=ic["qt"], u=ic["u"], v=ic["v"])
    return om, hm


CS_SIZE, CS_EXT = (24, 16, 20), dict(x=(0.0, 16e3), y=(0.0, 12e3), z=(0.0, 8e3))


def _cs_thb(z):
    return 300.0 + 0.0035 * z


def _cs_qvb(z):
    return float(0.013 * np.exp(-z / 2800.0))


def _cs_bub(x, y, z):
    return np.maximum(0.0, 1.0 - np.sqrt(((x - 8e3) / 4e3) ** 2 + ((y - 6e3) / 4e3) ** 2 + ((z - 1500.0) / 1500.0) ** 2))


def compressible_bubble(kessler=False, order=5):
    """tests/test_float32.py: the split-explicit bubble of the supercell example's precision, dry / Kessler, WENO5 / WENO9."""
    def build(orc, oc, bz, d):
        from oracle import oracle_compressible as ocm
        adv, need = _weno(order, d)
        base = 3 if order == 5 else 5
        og = orc.Grid(CS_SIZE, halo=_halo(3, base, need), **CS_EXT)
        om = ocm.CompressibleOracleModel(og, time_discretization=ocm.SplitExplicit(substeps=d.get("substeps", 6)), surface_pressure=1e5,
                                         reference_potential_temperature=_cs_thb, reference_vapor_mass_fraction=_cs_qvb,
                                         microphysics="Kessler" if kessler else None, advection=adv)
        th = lambda x, y, z: _cs_thb(z) + 2.0 * _cs_bub(x, y, z)
        qv = lambda x, y, z: np.vectorize(_cs_qvb)(z) + 0.003 * _cs_bub(x, y, z) + 0 * x + 0 * y
        x, y, z = og.nodes("ccc")
        rho = om.ref.density[og.Hz:og.Hz + og.Nz][:, None, None] * _cs_thb(z) / th(x, y, z)
        om.set(rho=rho, theta=th, u=5.0, v=0.0, w=0.0, qv=qv)
        hm = None
        if bz is not None:
            grid = bz.RectilinearGrid(CS_SIZE, halo=(base,) * 3, float_type=np.float32, **CS_EXT)
            dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), surface_pressure=1e5,
                                          reference_potential_temperature=_cs_thb, reference_vapor_mass_fraction=_cs_qvb)
            kw = dict(thermodynamic_constants=bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula()),
                      microphysics=bz.DCMIP2016KesslerMicrophysics()) if kessler else {}
            hm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=order), **kw)
            hm.set(ρ=rho, θ=th, u=5.0, v=0.0, w=0.0, qᵗ=qv)
        return om, hm
    return build


def _kessler_anelastic(orc, oc, bz, d):
    adv, need = _weno(5, d)
    size, extent = (16, 12, 20), ((0.0, 4e3), (0.0, 3e3), (0.0, 5e3))
    og = orc.Grid(size, x=extent[0], y=extent[1], z=extent[2], halo=_halo(3, 3, need))
    om = orc.OracleModel(og, surface_pressure=1e5, potential_temperature=300.0, microphysics="Kessler", advection=adv)
    bub = lambda x, y, z: np.maximum(0.0, 1.0 - np.sqrt((x - 2e3) ** 2 + (y - 1.5e3) ** 2 + (z - 1500.0) ** 2) / 1200.0)
    ic = dict(qt=lambda x, y, z: 0.016 * np.exp(-z / 3000.0) + 0.004 * bub(x, y, z), theta=lambda x, y, z: 300.0 + 0.004 * z + 1.0 * bub(x, y, z),
              qcl=lambda x, y, z: 0.003 * bub(x, y, z), qr=lambda x, y, z: 0.001 * bub(x, y, z), u=2.0)
    om.set(**ic)
    hm = None
    if bz is not None:
        grid = bz.RectilinearGrid(size, x=extent[0], y=extent[1], z=extent[2], float_type=np.float32)
        tc = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
        hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, tc, surface_pressure=1e5, potential_temperature=300.0)),
                                advection=bz.WENO(order=5), thermodynamic_constants=tc, microphysics=bz.DCMIP2016KesslerMicrophysics())
        hm.set(qᵗ=ic["qt"], θ=ic["theta"], qcl=ic["qcl"], qr=ic["qr"], u=ic["u"])
    return om, hm


def formulation_bubble(formulation):
    """tests/test_float32.py: a user tracer on the dry bubble (LiquidIcePotentialTemperature) / formulation = :StaticEnergy."""
    from helpers import bubble_theta

    def build(orc, oc, bz, d):
        adv, need = _weno(5, d)
        tr = formulation == "LiquidIcePotentialTemperature"
        og = orc.Grid((32, 20, 16), x=EXT[0], y=EXT[1], z=EXT[2], halo=_halo(3, 3, need))
        om = orc.OracleModel(og, potential_temperature=300.0, formulation=formulation, tracers=1 if tr else 0, advection=adv)
        th = bubble_theta(300.0, om.constants.g)
        a = lambda x, y, z: 1.0 + 0.5 * np.cos(2 * np.pi * y / 20e3) * (z / 10e3) + 0 * x
        om.set(theta=th, u=3.0, v=-2.0, **({"rc0": a} if tr else {}))
        hm = None
        if bz is not None:
            grid = bz.RectilinearGrid((32, 20, 16), x=EXT[0], y=EXT[1], z=EXT[2], float_type=np.float32)
            hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)), advection=bz.WENO(),
                                    formulation=formulation, tracers=("a",) if tr else ())
            if tr:
                hm.tracers["a"].set_interior(a)
            hm.set(θ=th, u=3.0, v=-2.0)
        return om, hm
    return build


def high_order_bubble(order):
    """tests/test_float32.py: the dry bubble under WENO(order = 7 / 9), halo 5."""
    from helpers import bubble_theta

    def build(orc, oc, bz, d):
        adv, need = _weno(order, d)
        og = orc.Grid((24, 16, 14), x=EXT[0], y=EXT[1], z=EXT[2], halo=_halo(3, 5, need))
        om = orc.OracleModel(og, potential_temperature=300.0, advection=adv)
        th = bubble_theta(300.0, om.constants.g)
        om.set(theta=th, u=3.0, v=-2.0)
        hm = None
        if bz is not None:
            grid = bz.RectilinearGrid((24, 16, 14), x=EXT[0], y=EXT[1], z=EXT[2], halo=(5, 5, 5), float_type=np.float32)
            hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)),
                                    advection=bz.WENO(order=order))
            hm.set(θ=th, u=3.0, v=-2.0)
        return om, hm
    return build


def _bounded_moisture(orc, oc, bz, d):
    import test_bounded_weno as tb
    from helpers import bubble_theta
    adv, need = _weno(5, d)
    size = (24, 24, 20)
    og = orc.Grid(size, x=tb.EXT[0], y=tb.EXT[1], z=tb.EXT[2], halo=_halo(3, 3, need))
    om = orc.OracleModel(og, potential_temperature=300.0, advection=adv)
    om.bounded = {"rq": (0.0, tb.QMAX)}
    th = bubble_theta(300.0, 9.81)
    om.set(theta=th, u=12.0, v=-7.0, qt=tb._blob)
    hm = None
    if bz is not None:
        grid = bz.RectilinearGrid(size, x=tb.EXT[0], y=tb.EXT[1], z=tb.EXT[2], float_type=np.float32)
        hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)),
                                advection={"momentum": bz.WENO(), "ρθ": bz.WENO(), "ρqᵛ": bz.WENO(bounds=(0.0, tb.QMAX))})
        hm.set(θ=th, u=12.0, v=-7.0, qᵗ=tb._blob)
    return om, hm


def _mixed_orders(orc, oc, bz, d):
    # the defect swaps the momentum order (9 -> 7); the scalars keep WENO5
    adv, need = _weno(9, d)
    size = (24, 24, 20)
    ext = dict(x=(0.0, 2400.0), y=(0.0, 2400.0), z=(0.0, 2000.0))
    og = orc.Grid(size, halo=(5, 5, 5), **ext)
    om = orc.OracleModel(og, potential_temperature=300.0, advection=adv, scalar_advection="WENO5")
    om.bounded = {"rq": (0.0, 1.0)}
    mask = lambda z: np.exp(-(z - 2000.0) ** 2 / (2 * 400.0 ** 2))
    om.relaxation = {"w": (0.125 * mask(og.zf), np.zeros(og.Nz + 1))}
    th = lambda x, y, z: 300.0 + 0.003 * z + 2.0 * np.exp(-((x - 1200.0) ** 2 + (y - 1200.0) ** 2 + (z - 1200.0) ** 2) / 300.0 ** 2)
    qt = lambda x, y, z: 0.004 * np.exp(-z / 1500.0) + 0 * x + 0 * y
    om.set(theta=th, u=4.0, v=-2.0, qt=qt)
    hm = None
    if bz is not None:
        grid = bz.RectilinearGrid(size, halo=(5, 5, 5), float_type=np.float32, **ext)
        hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)),
                                momentum_advection=bz.WENO(order=9), scalar_advection={"ρθ": bz.WENO(order=5), "ρqᵛ": bz.WENO(order=5, bounds=(0, 1))},
                                forcing={"w": bz.Relaxation(rate=0.125, mask=bz.GaussianMask(center=2000.0, width=400.0))})
        hm.set(θ=th, u=4.0, v=-2.0, qᵗ=qt)
    return om, hm


def _two_d_anelastic(orc, oc, bz, d):
    adv, need = _weno(5, d)
    topo = ("Periodic", "Flat", "Bounded")
    size, ext = (64, 48), dict(x=(-10e3, 10e3), z=(0.0, 10e3))
    og = orc.Grid(size, topology=topo, halo=_halo(2, 3, need), **ext)
    om = orc.OracleModel(og, potential_temperature=300.0, advection=adv)
    # a 10 K bubble: with 2 K the three steps move rho theta by too few Float32 ulps of its 300 K background to judge them
    θ = lambda x, z: 300.0 + 10.0 * np.cos(np.pi / 2 * np.minimum(1.0, np.hypot(x, z - 2000.0) / 2000.0)) ** 2
    om.set(theta=lambda x, y, z: θ(x, z) + 0 * y, u=2.0)
    hm = None
    if bz is not None:
        grid = bz.RectilinearGrid(size, topology=(bz.Periodic, bz.Flat, bz.Bounded), float_type=np.float32, **ext)
        hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)), advection=bz.WENO())
        hm.set(θ=θ, u=2.0)
    return om, hm


IGW = dict(Nx=96, Nz=10, Lx=96e3, Lz=10e3)


def _igw_theta_bg(z):
    return 300.0 * np.exp(1e-4 * z / 9.80665)


def _two_d_compressible(orc, oc, bz, d):
    from oracle import oracle_compressible as ocm
    adv, need = _weno(5, d)
    Nx, Nz, Lx, Lz = IGW["Nx"], IGW["Nz"], IGW["Lx"], IGW["Lz"]
    topo = ("Periodic", "Flat", "Bounded")
    # a 1 K wave (0.01 K moves rho_d, rho theta, rho u by a few Float32 ulps of their backgrounds in three steps: nothing to judge)
    θi = lambda x, z: _igw_theta_bg(z) + 1.0 * np.sin(np.pi * z / Lz) / (1 + (x - Lx / 3) ** 2 / 5000.0 ** 2)
    og = orc.Grid((Nx, Nz), x=(0.0, Lx), z=(0.0, Lz), topology=topo, halo=_halo(2, 3, need))
    td = ocm.SplitExplicit(substeps=d["substeps"]) if "substeps" in d else ocm.SplitExplicit()
    om = ocm.CompressibleOracleModel(og, time_discretization=td, reference_potential_temperature=_igw_theta_bg, reference_state=True, advection=adv)
    rho = om.ref.density[og.Hz:og.Hz + og.Nz][:, None, None] + np.zeros((Nz, 1, Nx))
    om.set(rho=rho, theta=lambda x, y, z: θi(x, z) + 0 * y, u=20.0, v=0.0, w=0.0)
    hm = None
    if bz is not None:
        grid = bz.RectilinearGrid((Nx, Nz), x=(0.0, Lx), z=(0.0, Lz), topology=(bz.Periodic, bz.Flat, bz.Bounded), float_type=np.float32)
        dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(), reference_potential_temperature=_igw_theta_bg, reference_state="auto")
        hm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO())
        hm.set(ρ=rho, θ=θi, u=20.0, v=0.0, w=0.0)
    return om, hm


# the compressible Kessler bubble that the y-slab test decomposes (device vs device: the oracle side serves the CPU tolerance test)
SLAB_SIZE, SLAB_EXT = (32, 24, 16), ((-4e3, 4e3), (-3e3, 3e3), (0.0, 8e3))


def slab_theta(x, y, z):
    return 300.0 + 2.0 * np.maximum(0.0, 1.0 - np.sqrt(x ** 2 + y ** 2 + (z - 3000.0) ** 2) / 2000.0)


def slab_qv(x, y, z):
    return 5e-3 * np.exp(-z / 2e3) * (1 + 0.2 * np.sin(2 * np.pi * x / 8e3)) + 0 * y


def _slab_compressible_oracle(orc, oc, bz, d):
    from oracle import oracle_compressible as ocm
    adv, need = _weno(5, d)
    og = orc.Grid(SLAB_SIZE, x=SLAB_EXT[0], y=SLAB_EXT[1], z=SLAB_EXT[2], halo=_halo(3, 3, need))
    om = ocm.CompressibleOracleModel(og, time_discretization=ocm.SplitExplicit(substeps=d.get("substeps", 6)), reference_potential_temperature=300.0,
                                     microphysics="Kessler", advection=adv)
    rho = om.ref.density[og.Hz:og.Hz + og.Nz][:, None, None]
    om.set(rho=rho, theta=slab_theta, u=3.0, v=-2.0, w=0.0, qv=slab_qv)
    return om, None


# Float32 substep storage in a Float64 compressible model (tests/test_gpu_compressible.py): the oracle side of its six variants
SUBSTEP_TD = [dict(substeps=6), dict(), dict(substeps=4, damping_coefficient=0.05, damp_vertical=True),
              dict(substeps=6, damping_coefficient=None), dict(substeps=6, sponge=(0.2, 3000.0, "cubic")),
              dict(substeps=8, substep_distribution="constant")]


def substep_storage_theta(x, y, z):
    r = np.sqrt(x ** 2 + y ** 2 + (z - 3000.0) ** 2)
    return 300.0 + 2.0 * np.maximum(0.0, 1.0 - r / 2000.0)


def substep_storage_qv(x, y, z):
    return 5e-3 * np.exp(-z / 2e3) * (1 + 0.2 * np.sin(2 * np.pi * x / 8e3)) + 0 * y


def _substep_storage(td):
    def build(orc, oc, bz, d):
        from oracle import oracle_compressible as ocm
        from test_gpu_compressible import EXTENT
        t = dict(td)
        if "substeps" in d and t.get("substeps"):
            t["substeps"] = t["substeps"] - 1
        og = orc.Grid((24, 16, 24), x=EXTENT["x"], y=EXTENT["y"], z=EXTENT["z"])
        om = ocm.CompressibleOracleModel(og, time_discretization=ocm.SplitExplicit(**t), reference_potential_temperature=300.0, reference_state=True)
        rho = om.ref.density[og.Hz:og.Hz + og.Nz][:, None, None]
        u0 = lambda x, y, z: 3.0 + 0 * x + 0 * y + 0 * z
        om.set(rho=rho, theta=substep_storage_theta, u=u0, v=0.0, w=0.0, qv=substep_storage_qv)
        return om, None
    return build


ANELASTIC_ALL = ("ru", "rv", "rw", "rtheta", "rq", "T")
COMPRESSIBLE_ALL = ("rho_d", "rtheta", "rq", "T", "p", "ru", "rw")

# the set-ups of tests/test_float32.py (name -> Case)
STEP_CASES = {
    "bomex": Case("bomex", "anelastic", ANELASTIC_ALL, 3.0, 3, _bomex, defects=("dt", "weno")),
    "compressible_dry": Case("compressible_dry", "compressible", COMPRESSIBLE_ALL, 2.0, 2, compressible_bubble(False), defects=("dt", "substeps")),
    "compressible_kessler": Case("compressible_kessler", "compressible", COMPRESSIBLE_ALL, 2.0, 2, compressible_bubble(True), defects=("dt", "substeps")),
    # the cloud water of this set-up evaporates within the first step in both models (rho q^cl ends at zero: no increment to judge), and
    # T follows that evaporation's cooling more than the step length: neither defect moves it by three tolerances, so T is left to the
    # test's own field-scale check
    "kessler": Case("kessler", "anelastic", ("ru", "rw", "rtheta", "rq", "rqr"), 5.0, 2, _kessler_anelastic, defects=("dt", "weno")),
    "tracer": Case("tracer", "anelastic", ("ru", "rv", "rw", "rtheta", "rc0"), 2.0, 3, formulation_bubble("LiquidIcePotentialTemperature"),
                   defects=("dt", "weno")),
    "static_energy": Case("static_energy", "anelastic", ("ru", "rv", "rw", "rtheta"), 2.0, 3, formulation_bubble("StaticEnergy"), defects=("dt", "weno")),
    "weno7": Case("weno7", "anelastic", ("ru", "rv", "rw", "rtheta"), 2.0, 3, high_order_bubble(7), defects=("dt", "weno")),
    "weno9": Case("weno9", "anelastic", ("ru", "rv", "rw", "rtheta"), 2.0, 3, high_order_bubble(9), defects=("dt", "weno")),
    "compressible_weno9_kessler": Case("compressible_weno9_kessler", "compressible", ("rho_d", "rtheta", "rq", "T", "ru", "rw"), 2.0, 2,
                                       compressible_bubble(True, order=9), defects=("dt", "weno", "substeps")),
    "slabs": bubble_case("slabs", (32, 24, 16)),
    "bounded_moisture": Case("bounded_moisture", "anelastic", ANELASTIC_ALL[:5], 5.0, 3, _bounded_moisture, defects=("dt", "weno")),
    "slab_compressible": Case("slab_compressible", "compressible", ("rho_d", "ru", "rw", "rtheta", "rq"), 2.0, 2, _slab_compressible_oracle,
                              defects=("dt", "substeps")),
    "two_d_anelastic": Case("two_d_anelastic", "anelastic", ("ru", "rw", "rtheta"), 2.0, 3, _two_d_anelastic, defects=("dt", "weno")),
    "two_d_compressible": Case("two_d_compressible", "compressible", ("rho_d", "rtheta", "ru"), 6.0, 3, _two_d_compressible, defects=("dt",)),
    "mixed_orders": Case("mixed_orders", "anelastic", ANELASTIC_ALL[:5], 3.0, 3, _mixed_orders, defects=("dt", "weno")),
}
for _size in ((32, 20, 16), (64, 24, 16), (64, 16, 32)):
    for _moist in (False, True):
        _c = bubble_case("time_steps_%dx%dx%d_%s" % (_size + ("moist" if _moist else "dry",)), _size, moist=_moist)
        STEP_CASES[_c.name] = _c

SUBSTEP_CASES = {f"substep_storage_{i}": Case(f"substep_storage_{i}", "substep_storage", ("rho_d", "rtheta", "rq", "ru", "rv", "rw", "T", "p"),
                                              2.0, 3, _substep_storage(td), defects=("dt", "substeps") if td.get("substeps") else ("dt",))
                 for i, td in enumerate(SUBSTEP_TD)}


# ---- the Float32 lean-seam sweep (tests/test_float32_increments.py) -------------------------------------------------------------------------------
def lean_chunks(Nx, Ny, nlev, TY=8):
    """pick_chunk5 of csrc/bz_tendency5.hip on the coarse rule (the Float32 twin): (chunk length, number of z chunks)."""
    tiles = ((Nx + 63) // 64) * ((Ny + TY - 1) // TY)
    want = min((1024 + tiles - 1) // tiles, max(nlev // 128, 1))
    want = max(want, 1)
    if tiles * want < 512:
        fill = (512 + tiles - 1) // tiles
        cap = max(nlev // 8, 1)
        if tiles * cap < 256:
            cap = max(nlev // 2, 1)
        want = max(want, min(fill, cap))
    kc = (nlev + want - 1) // want
    return kc, (nlev + kc - 1) // kc


def lean_xcd(Nx, Ny, nlev, TY=8):
    """XCD block order of a lean launch (grid.x * grid.y * grid.z divisible by 8) for `nlev` levels."""
    return ((Nx + 63) // 64) * ((Ny + TY - 1) // TY) * lean_chunks(Nx, Ny, nlev, TY)[1] % 8 == 0


SWEEP_CASES = {c.name: c for c in (
    # Nx < 64, Ny % 8 != 0 (a partial last tile row), three tile rows; rocFFT x transforms (Ny % 8 != 0)
    bubble_case("nx32_ny20", (32, 20, 16)),
    # Nx % 64 != 0 (two x tiles, the second partial), two tile rows (< 3), moist
    bubble_case("nx72_ny12_moist", (72, 12, 12), moist=True),
    # Nx = 130: three x tiles, the last of two columns; the scalar kernel's grid 3 x 2 x 6 is not a multiple of 8 (hardware order) ...
    bubble_case("nx130_ny16", (130, 16, 12)),
    # ... and the same case with the XCD order switched off everywhere
    bubble_case("nx130_ny16_noxcd", (130, 16, 12), env={"BZ_NO_XCD": "1"}),
    # Nx a multiple of 64, Ny % 8 == 0: the hand-written x transforms of the Poisson solve, moist
    bubble_case("nx64_ny24_moist", (64, 24, 16), moist=True),
    # Nx a multiple of 64 with flow from the east across a bubble on the periodic seam: the upwind stencils of the last column reach
    # into the east halo, which the east frame loads of the last full tile bring in
    bubble_case("nx64_ny24_westward_moist", (64, 24, 16), moist=True, u=-3.0, v=2.0, seam=10.0),
    # the kx-major spectrum with a chunked middle (32 KB chunks) in Float32
    bubble_case("nx64_ny16_kxchunk", (64, 16, 32), env={"BZ_POISSON_KX_CHUNK_KB": "32"}),
    # a stretched z grid, moist
    bubble_case("stretched_moist", (32, 24, 16), moist=True, stretched=True),
    # (Periodic, Bounded, Bounded): the WY instantiations of the lean kernels (the cosine-transform solve needs Ny % 8 == 0)
    bubble_case("walls_y", (32, 24, 16), topology=("Periodic", "Bounded", "Bounded")),
    # the lean forcing epilogues: FPlane + geostrophic u / v profiles, no closure (bzi_lean_forcings_ok), moist
    bubble_case("coriolis_geostrophic_moist", (32, 24, 16), moist=True, forcings=True),
)}

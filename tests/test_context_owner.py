"""What every model class inherits from the owner of a context (breeze.jl_amd/_context.py: ContextOwner): synchronize, the profile, the
graph switch, comm_info and the release of the context — on each of the five model classes, the slab ones as the single rank of an
in-process communicator (transport "local:<name>") and SlabAtmosphereModel also over its own torch orchestration, which needs no
process group at world = 1."""
import gc
import uuid

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXT = dict(x=(0.0, 16e3), y=(0.0, 8e3), z=(0.0, 8e3))


def theta(x, y, z):
    return 300.0 + 0.004 * z + 2.0 * np.exp(-((x - 8e3) ** 2 + (y - 4e3) ** 2 + (z - 2e3) ** 2) / 2e3 ** 2)


def local():
    return "local:" + uuid.uuid4().hex


def anelastic(bz, **kw):
    g = bz.RectilinearGrid((16, 8, 8), **EXT)
    m = bz.AtmosphereModel(g, dynamics=bz.AnelasticDynamics(bz.ReferenceState(g, potential_temperature=300.0)), advection=bz.WENO(order=5), **kw)
    m.set(θ=theta, u=2.0)
    return m


def kinematic(bz):
    g = bz.RectilinearGrid((16, 8, 8), **EXT)
    m = bz.AtmosphereModel(g, dynamics=bz.PrescribedDynamics(bz.ReferenceState(g, potential_temperature=300.0)), advection=bz.WENO(order=5))
    m.set(θ=theta, u=2.0)
    return m


def compressible(bz, slab=False):
    g = bz.RectilinearGrid((16, 8, 8), **EXT)
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), surface_pressure=1e5, reference_potential_temperature=300.0)
    if slab:
        m = bz.compressible.SlabCompressibleModel(g, 0, 1, dyn, advection=bz.WENO(order=5), transport=local(), device="cuda:0")
    else:
        m = bz.CompressibleAtmosphereModel(g, dyn, advection=bz.WENO(order=5))
    ρ = m.dynamics.reference_state.density[g.Hz:g.Hz + g.Nz][:, None, None]
    m.set(ρ=ρ, θ=theta, u=2.0, v=0.0, w=0.0)
    return m


def slab(bz, cls, transport):
    from breeze_jl_amd import distributed
    g = bz.RectilinearGrid((16, 8, 8), **EXT)
    m = getattr(distributed, cls)(g, 0, 1, transport=transport, potential_temperature=300.0, advection=bz.WENO(order=5), device="cuda:0")
    m.set(θ=theta, u=2.0)
    return m


# name -> (factory, whether the context has a library-owned communicator)
MODELS = {
    "AtmosphereModel": (anelastic, False),
    "AtmosphereModel-kinematic": (kinematic, False),
    "CompressibleAtmosphereModel": (compressible, False),
    "SlabAtmosphereModel-local": (lambda bz: slab(bz, "SlabAtmosphereModel", local()), True),
    "SlabAtmosphereModel-torch": (lambda bz: slab(bz, "SlabAtmosphereModel", "torch"), False),
    "LibrarySlabAtmosphereModel-local": (lambda bz: slab(bz, "LibrarySlabAtmosphereModel", local()), True),
    "SlabCompressibleModel-local": (lambda bz: compressible(bz, slab=True), True),
}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_context_owner(bz, name):
    make, has_communicator = MODELS[name]
    m = make(bz)
    assert isinstance(m, bz._context.ContextOwner) and m._ctx and m._T.ftype == 8
    m.time_step(2.0)
    assert m.synchronize() is None
    assert m.graph_info() == (False, 0, 0)
    if name == "AtmosphereModel-kinematic":
        with pytest.raises(NotImplementedError, match="hipGraph replay is not implemented"):
            m.graph_enable()
        assert m.graph_info() == (False, 0, 0)
    m.profile_enable()
    m.profile_reset()
    m.time_step(2.0)
    m.synchronize()
    profile = m.profile()
    assert profile and all(type(k) is str and type(ms) is float and type(n) is int for k, (ms, n) in profile.items())
    assert any(n > 0 for _, n in profile.values())
    if has_communicator:
        transport, sent, exchanges = m.comm_info()
        assert (type(transport), type(sent), type(exchanges)) == (str, int, int)
    else:      # no library-owned communicator on this context: the library says so, nothing is returned
        with pytest.raises(bz.BreezeHIPError, match="bz_comm_info"):
            m.comm_info()
    assert np.isfinite(m.potential_temperature_density.interior_cpu()).all()
    # the context is released exactly once
    m.__del__()
    assert m._ctx is None
    m.__del__()
    del m
    gc.collect()
    again = make(bz)
    again.time_step(2.0)
    again.synchronize()
    assert np.isfinite(again.potential_temperature_density.interior_cpu()).all()
    del again
    gc.collect()

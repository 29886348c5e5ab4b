"""The launch census of the single-domain substep: for a table of named configurations, which kernels two Runge-Kutta substeps launch and how often,
read off the library's own profile (tlab_profile_report).  tests/test_gpu_launch_census.py holds every case to the record in
tests/golden/launch_census.json, so an edit of the route decisions in tlab_amd/csrc/rhs.cpp is checked against a record instead of by eye.

    python tests/launch_census.py            writes tests/golden/launch_census.json (on the GPU; the record is made from the commit BEFORE a change)
    python tests/launch_census.py --digest F   also writes the SHA-256 of q, s, hq, hs of every case after its two substeps to F (two builds that
                                               launch the same kernels with the same arguments give the same bits)

The census counts launches per tag; it does not see their arguments.  TEST INFRASTRUCTURE."""
import ctypes
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cases as C      # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "launch_census.json")
REF_HYPER = 0.1        # the wall closure of tests/test_gpu_rhs.py
FAST, SMALL = (256, 64, 64), (32, 40, 16)      # the fast kernels apply / they do not
DTIME = 2e-3
FREESLIP = ("freeslip", "freeslip", "neumann", "neumann")
CLOUD = dict(mixture=(-2.5, 0.8, 0.0), infrared=("grayliquid", 2, 3.0, -4.0, 1.5),
             buoyancy={"type": "linear", "vector": (0.0, -2.0, 0.0), "scalars": 3, "parameters": (1.0, -0.4, 0.9, 0.1), "inb_scal_array": 3})
FORCES = dict(coriolis={"type": "explicit", "vector": (0.0, 1.5, 0.0)}, buoyancy={"type": "linear", "vector": (0.0, -2.0, 0.0), "parameters": (1.0, 0.1)})
ZONES = dict(points_jmin=5, points_jmax=8, params_u=(150.0, 2.0), params_s=(120.0, 2.0))

# name -> what differs from the default (256 x 64 x 64, stretched y, no-slip walls, one Dirichlet scalar, fused).  Keys: shape, nscal, fuse, walls
# (the four keywords of Dns.set_bcs), env (TLAB_NEUMANN_PLANES; None: unset), anelastic, pfilter, dealias, stagger, remove_divergence, surface, zones,
# bounds, forces, cloud, rhs_only.  The comment names the route the case is there for.
CASES = {
    "default": {},                                                        # div_all: the five Burgers launches with the forcing terms on them
    "unfused": dict(fuse=False),                                          # the per-equation literal Burgers sums on the fast kernels' shape
    "small": dict(shape=SMALL),                                           # ... where no fast kernel applies
    "small_unfused": dict(shape=SMALL, fuse=False),
    "nscal0": dict(nscal=0),                                              # one batch of three
    "nscal5": dict(nscal=5),                                              # batches of four: 4 + 4
    "nz1": dict(shape=(256, 64, 1)),                                      # no z Burgers launch to batch: per-equation sums, x and y fused, z through a temporary
    "nx1024": dict(shape=(1024, 64, 16)),                                 # x lines beyond the wave-per-line Burgers kernel: per-equation sums, the three fused forcing launches (y first)
    "nz2048": dict(shape=(16, 32, 2048)),                                 # nx below the fast kernels, long z lines
    "freeslip_neumann": dict(walls=FREESLIP),                             # Neumann fast tail, wall planes from weighted sums
    "freeslip_neumann_planes0": dict(walls=FREESLIP, env="0"),            # ... from the derivative pass along y
    "one_wall": dict(walls=("noslip", "freeslip", "dirichlet", "dirichlet")),       # the one-wall variant, Dirichlet scalar finished by the x launch
    "one_wall_planes0": dict(walls=("noslip", "freeslip", "dirichlet", "dirichlet"), env="0"),
    "freeslip_dirichlet_scalar_nscal2": dict(walls=("freeslip", "freeslip", "neumann", "dirichlet"), nscal=2),
    "freeslip_small": dict(shape=SMALL, walls=FREESLIP),                  # the slow Neumann tail: sub3, BOUNDARY_BCS_NEUMANN_Y, final_update
    "freeslip_unfused": dict(walls=FREESLIP, fuse=False),
    "anelastic": dict(anelastic=True),                                    # literal with batched Burgers, axpy3w, the deferred density weight
    "anelastic_freeslip": dict(anelastic=True, walls=("freeslip", "freeslip", "neumann", "dirichlet")),
    "anelastic_unfused": dict(anelastic=True, fuse=False),
    "pressure_filter": dict(pfilter=True),
    "pressure_filter_freeslip": dict(pfilter=True, walls=FREESLIP),
    "dealiasing_y": dict(dealias=True),                                   # literal, per-equation Burgers through OPR_Burgers
    "stagger": dict(stagger=True),                                        # literal with batched Burgers, the forcing and the gradient on the pressure nodes
    "stagger_small": dict(stagger=True, shape=SMALL),
    "no_remove_divergence": dict(remove_divergence=False),
    "surface": dict(surface=True),
    "surface_small": dict(surface=True, shape=SMALL),
    "zones_dirichlet": dict(zones=True),                                  # zone_epi: the scalar zone in the mid-sequence slot, wall planes by the plane form
    "zones_neumann": dict(zones=True, walls=FREESLIP),                    # zone_tail inside the Neumann fast tail
    "zones_small": dict(zones=True, shape=SMALL),                         # zone_tail in the literal tail
    "zones_anelastic": dict(zones=True, forces=True, anelastic=True),     # the mid-sequence slot of the three-launch form (after its first launch)
    "zones_nx1024": dict(zones=True, forces=True, shape=(1024, 64, 16)),
    "zones_nz1": dict(zones=True, shape=(256, 64, 1)),
    "bounds_dirichlet": dict(bounds=True),                                # clip mode 1
    "bounds_neumann": dict(bounds=True, walls=FREESLIP),                  # clip mode 2
    "bounds_neumann_planes0": dict(bounds=True, walls=FREESLIP, env="0"),  # k_clip after the y-line tail
    "bounds_zones_dirichlet": dict(bounds=True, zones=True),
    "body_forces": dict(forces=True),
    "body_forces_small": dict(forces=True, shape=SMALL),
    "cloud": dict(cloud=True, nscal=2),                                   # mixture + buoyancy on the liquid + infrared source
    "cloud_small": dict(cloud=True, nscal=2, shape=SMALL),
    "rhs_only_noslip": dict(rhs_only=True),
    "rhs_only_freeslip": dict(rhs_only=True, walls=FREESLIP),
    "rhs_only_small_freeslip": dict(rhs_only=True, walls=FREESLIP, shape=SMALL),
}


def _filters():
    return np.load(os.path.join(HERE, "golden", "filters.npz"))


def _device_filter(T, key):
    G = _filters()
    n, t, per, b0, b1 = (int(v) for v in re.match(r"n(\d+)_t(\d+)_p(\d)_b(\d)(\d)", key).groups())
    c = G[key + "_coeffs"]
    return T.Filter(t, n, bool(per), c if c.shape[1] else None, b0, b1)


def report():
    """{tag: calls} of the library's profile since the last tlab_profile_reset"""
    from tlab_amd.lib import load
    buf = ctypes.create_string_buffer(1 << 16)
    load().tlab_profile_report(buf, len(buf))
    return {r.split("\t")[0]: int(r.split("\t")[1]) for r in buf.value.decode().splitlines() if "\t" in r}


def run(name, setenv=None, delenv=None):
    """({tag: calls}, [q, s, hq, hs as numpy arrays]) of case `name` after begin_step and two substeps.  setenv(key, value) / delenv(key) change the
    environment (a test passes monkeypatch's; default: os.environ itself)."""
    import torch
    import tlab_amd as T
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load
    case = CASES[name]
    setenv = setenv or os.environ.__setitem__
    delenv = delenv or (lambda k: os.environ.pop(k, None))
    if case.get("env") is None:
        delenv("TLAB_NEUMANN_PLANES")
    else:
        setenv("TLAB_NEUMANN_PLANES", case["env"])
    T.init(0)
    nx, ny, nz = case.get("shape", FAST)
    nscal = case.get("nscal", 1)
    walls = case.get("walls")
    x, y, z = C.grids(nx, ny, nz, True)
    if walls and walls[0] == "freeslip" and walls[1] == "freeslip":
        q0, s0 = C.neumann_fields(x, y, z, 21)
    else:
        q0, s0 = C.init_fields(nx, ny, nz, x, y, z, 3)
    ss = [s0[0] * (1.0 + 0.3 * i) + 0.1 * i for i in range(nscal)]
    sc = (0.7, 1.0, 2.5, 0.5, 1.5)[:nscal]
    L = load()
    keep = []
    d = Dns(x, y, z, nscal=nscal, visc=1.0 / 800.0, schmidt=sc if nscal else (1.0,), yuniform=False, hyper_bc1_ext=REF_HYPER, stagger=bool(case.get("stagger")))
    try:
        d.set_fusion(case.get("fuse", True))
        if walls:
            d.set_bcs(*walls)
        if case.get("anelastic"):
            d.set_anelastic(1.0 + 0.6 * np.exp(-2.5 * (y - y[0]) / (y[-1] - y[0])))
        if case.get("pfilter"):
            keep.append(_device_filter(T, "n64_t1_p0_b66"))
            d.set_pressure_filter(None, keep[-1], None)
        if case.get("dealias"):
            keep.append(_device_filter(T, "n64_t1_p0_b11"))
            T.set_dealiasing(2, keep[-1])
        if not case.get("remove_divergence", True):
            d.set_remove_divergence(False)
        if case.get("surface"):
            d.set_surface_bcs(["linear"], ["static"], [0.35], [-0.2])
        if case.get("cloud"):
            d.set_mixture("airwaterlinear", CLOUD["mixture"])
            d.set_body_forces(None, CLOUD["buoyancy"])
            d.set_infrared(*CLOUD["infrared"])
        if case.get("forces"):
            d.set_body_forces(FORCES["coriolis"], FORCES["buoyancy"])
        for i in range(3):
            d.q[i].copy_(torch.from_numpy(q0[i]))
        for i in range(nscal):
            d.s[i].copy_(torch.from_numpy(ss[i]))
        if d.liquid is not None:
            d.FI_DIAGNOSTIC()
        if case.get("zones"):
            d.set_buffer_zones(**ZONES)      # (the reference fields are the plane means of the fields loaded above)
        if case.get("bounds"):
            d.set_scalar_bounds([-0.2] * nscal, [0.6] * nscal)
        torch.cuda.synchronize()
        L.tlab_profile_reset(); L.tlab_profile_enable(1)
        d.begin_step()
        for k in range(2):      # the first on fresh tendencies, the second accumulating
            if case.get("rhs_only"):
                d.RHS_GLOBAL_INCOMPRESSIBLE_1(DTIME * d.kdt[k])
            else:
                d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(DTIME * d.kdt[k], d.kco[k], True)
        torch.cuda.synchronize()
        L.tlab_profile_enable(0)
        counts = report()
        L.tlab_profile_reset()
        return counts, [t.cpu().numpy().copy() for t in d.q + d.s + d.hq + d.hs]
    finally:
        L.tlab_profile_enable(0)
        if case.get("anelastic"):
            d.set_anelastic(None)
        if case.get("dealias"):
            T.set_dealiasing(2, None)


def census(name, setenv=None, delenv=None):
    return run(name, setenv, delenv)[0]


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def main(argv):
    out, digest = GOLDEN, None
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
    if "--digest" in argv:
        digest = argv[argv.index("--digest") + 1]
    table, failed, sums = {}, [], {}
    for name in CASES:
        try:
            table[name], fields = run(name)
        except Exception as e:       # noqa: BLE001  (nothing more runs on the device after a failure; the record is written only when all ran)
            print("FAILED", name, repr(e), flush=True)
            failed.append(name)
            break
        print(name, json.dumps(table[name], sort_keys=True), flush=True)
        sums[name] = [hashlib.sha256(a.tobytes()).hexdigest() for a in fields]
    os.environ.pop("TLAB_NEUMANN_PLANES", None)
    if digest:
        with open(digest, "w") as f:
            json.dump(sums, f, indent=1, sort_keys=True)
    if failed:
        print("not written, failed cases:", failed)
        return 1
    with open(out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

#!/usr/bin/env python3
"""Golden vectors for the Multipole: tests/golden/dkd_multipole.npz.

Run in the build container only (imports the reference read-only through generate_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_golden_dkd_multipole.py

The reference has no thin multipole. Its Bmad-X module has the building blocks, and this script composes the map from them in
float64 (DATA only in the file: inputs, parameters, outputs):

    cheetah_to_bmad_coords                          (tau, delta) -> (z, pz), once
    offset_particle_set(misalignment, tilt)
    track_a_drift(h),  h = L / (2 n)
    n x [ w = (knl + i ksl) / n (x + i y)^m / m!,  px -= Re w,  py += Im w;  track_a_drift(2 h), h behind the last kick ]
    offset_particle_unset
    bmad_to_cheetah_coords                          (z, pz) -> (tau, delta), once

(x + i y)^m is built by m complex multiplications from 1 in real arithmetic (Horner), the order the kernel uses. The script also
evaluates every case with torch's complex power instead and prints the spread between the two orderings of the same arithmetic:
what a comparison against these vectors cannot resolve.

Cases: each order m = 0 .. 3 with both strengths non-zero, once thin (length = 0, one kick) and once thick; upright, tilted,
misaligned and both; num_steps 1 and 3. The beams are the sextupole generator's (the same seed and construction): 257 electrons
at 100 MeV, sigma_x = sigma_y = 1 mm and 5 mm, sigma_delta = 2e-3.
"""

import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from generate_golden import cheetah, np, npy, save, species_meta, torch  # noqa: E402

from cheetah.utils import bmadx  # noqa: E402

F64 = {"dtype": torch.float64}
N = 257


def t64(v):
    return torch.tensor(v, **F64)


def dkd_multipole(particles, energy, mc2, length, order, knl, ksl, tilt, misalignment, num_steps, horner=True):
    """The map of the module docstring on (N, 7) particles; returns ((N, 7) particles, outgoing reference energy)."""
    q, p0c = bmadx.cheetah_to_bmad_coords(particles, energy, mc2)
    x, px, y, py, z, pz = (q[..., j] for j in range(6))
    x, px, y, py = bmadx.offset_particle_set(misalignment[0], misalignment[1], tilt, x, px, y, py)
    h = length / (2 * num_steps)
    bn, an = knl / math.factorial(order) / num_steps, ksl / math.factorial(order) / num_steps
    x, y, z = bmadx.track_a_drift(h, x, px, y, py, z, pz, p0c, mc2)
    for step in range(num_steps):
        if horner:
            re, im = torch.ones_like(x), torch.zeros_like(x)
            for _ in range(order):
                re, im = re * x - im * y, re * y + im * x
        else:
            w = torch.complex(x, y) ** order
            re, im = w.real, w.imag
        px = px - (bn * re - an * im)
        py = py + (bn * im + an * re)
        x, y, z = bmadx.track_a_drift(2 * h if step + 1 < num_steps else h, x, px, y, py, z, pz, p0c, mc2)
    x, px, y, py = bmadx.offset_particle_unset(misalignment[0], misalignment[1], tilt, x, px, y, py)
    out, ref_energy = bmadx.bmad_to_cheetah_coords(torch.stack([x, px, y, py, z, pz], dim=-1), p0c, mc2)
    return torch.cat([out[..., :6], torch.ones_like(out[..., :1])], dim=-1), ref_energy


def main():
    species = cheetah.Species("electron", **F64)
    energy = t64(1e8)
    arrays = {"energy": npy(energy), "species": np.asarray(species_meta(species))}
    g = torch.Generator().manual_seed(20)
    beams = {}
    for tag, sigma in (("1mm", 1e-3), ("5mm", 5e-3)):
        x = torch.randn(N, 7, generator=g, **F64) * t64([sigma, 2e-5, sigma, 2e-5, 1e-4, 2e-3, 0.0])
        x[:, 6] = 1.0
        beams[tag] = x
        arrays[f"in_{tag}"] = npy(x)
    cases = [  # name, length, order, knl, ksl, tilt, misalignment, num_steps
        ("order0_thin_upright_n1", 0.0, 0, 1e-4, -2e-4, 0.0, [0.0, 0.0], 1),
        ("order1_thin_tilted_n1", 0.0, 1, 0.6, -0.3, 0.3, [0.0, 0.0], 1),
        ("order2_thin_misaligned_n1", 0.0, 2, 20.0, -12.0, 0.0, [1e-3, -5e-4], 1),
        ("order3_thin_tilted_misaligned_n1", 0.0, 3, 2e4, -1e4, -0.4, [1e-3, -5e-4], 1),
        ("order0_tilted_n3", 0.25, 0, -2e-4, 1e-4, 0.3, [0.0, 0.0], 3),
        ("order1_misaligned_n3", 0.2, 1, -0.4, 0.5, 0.0, [1e-3, -5e-4], 3),
        ("order2_upright_n1", 0.2, 2, 20.0, -12.0, 0.0, [0.0, 0.0], 1),
        ("order3_tilted_misaligned_n3", 0.25, 3, -2e4, 1.5e4, -0.4, [1e-3, -5e-4], 3),
    ]
    spread = 0.0
    for name, length, order, knl, ksl, tilt, mis, n in cases:
        arrays[f"{name}_params"] = np.asarray([length, knl, ksl, tilt, mis[0], mis[1]])
        arrays[f"{name}_order"] = np.asarray(order)
        arrays[f"{name}_steps"] = np.asarray(n)
        for tag, x in beams.items():
            args = (x, energy, species.mass_eV, t64(length), order, t64(knl), t64(ksl), t64(tilt), t64(mis), n)
            out, e_out = dkd_multipole(*args)
            other, _ = dkd_multipole(*args, horner=False)
            drift, _ = dkd_multipole(x, energy, species.mass_eV, t64(length), order, t64(0.0), t64(0.0), t64(tilt), t64(mis), n)
            arrays[f"{name}_{tag}_out"] = npy(out)
            arrays[f"{name}_{tag}_energy_out"] = npy(e_out)
            moved = ((out - drift).abs().amax(dim=0) / out.abs().amax(dim=0))[:4]
            s = float(((out - other).abs().amax(dim=0) / out.abs().amax(dim=0))[:6].max())
            spread = max(spread, s)
            print(name, tag, "the kicks move x, px, y, py by", [f"{float(m):.1e}" for m in moved], "of the column's largest magnitude;",
                  f"Horner against the complex power: {s:.1e}")
    print(f"largest spread between the two orderings: {spread:.2e} of a column's largest magnitude",
          "(below 1e-13: the bound 1e-12 stands)" if spread <= 1e-13 else "(ABOVE 1e-13: widen the bound to ten times the spread)")
    arrays["names"] = np.asarray([c[0] for c in cases])
    arrays["beams"] = np.asarray(list(beams))
    save("dkd_multipole.npz", **arrays)


if __name__ == "__main__":
    main()

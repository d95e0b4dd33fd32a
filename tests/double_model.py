"""A numpy float64 model of the reference's timestep, av_velocity and write_values quantities: SerialCode/d2q9-bgk.c
:207-458 and :684-719 with every `float` read as `double`, `sqrtf` as `sqrt` and every `1.f`-style literal as a double
literal, in the reference's own operation order (each numpy ufunc rounds once, as each C operator does; numpy never
contracts a*b+c).  It is what the double engine (lbm_double_*) is compared with bit for bit, and tests/test_double_model.py
pins it to the reference's golden results.  The one liberty: av_velocity adds the cells' |u| with numpy's pairwise sum,
not sequentially (a difference near 1e-15 relative; the tests' bounds say where it enters).

Arrays: cells (ny, nx, 9) float64 in the reference's AoS layout, obstacles (ny, nx) with nonzero = blocked.
"""
import numpy as np

C_SQ = 1.0 / 3.0          # :308
W0 = 4.0 / 9.0            # :309
W1 = 1.0 / 9.0            # :310
W2 = 1.0 / 36.0           # :311


def init_cells(nx, ny, density):
    """initialise() :546-567."""
    density = float(density)
    cells = np.empty((ny, nx, 9), dtype=np.float64)
    cells[..., 0] = density * 4.0 / 9.0
    cells[..., 1:5] = density / 9.0
    cells[..., 5:9] = density / 36.0
    return cells


def accelerate_flow(cells, blocked, density, accel):
    """:216-246, in place on row ny - 2."""
    w1 = float(density) * float(accel) / 9.0
    w2 = float(density) * float(accel) / 36.0
    row = cells[cells.shape[0] - 2]
    go = (~blocked[cells.shape[0] - 2]) & ((row[:, 3] - w1) > 0.0) & ((row[:, 6] - w2) > 0.0) & ((row[:, 7] - w2) > 0.0)
    row[go, 1] += w1
    row[go, 5] += w2
    row[go, 8] += w2
    row[go, 3] -= w1
    row[go, 6] -= w2
    row[go, 7] -= w2


def propagate(cells):
    """:248-277: tmp[jj, ii, k] = cells at the neighbour speed k arrives from, periodic."""
    tmp = np.empty_like(cells)
    tmp[..., 0] = cells[..., 0]
    tmp[..., 1] = np.roll(cells[..., 1], 1, axis=1)                        # from x_w
    tmp[..., 2] = np.roll(cells[..., 2], 1, axis=0)                        # from y_s
    tmp[..., 3] = np.roll(cells[..., 3], -1, axis=1)                       # from x_e
    tmp[..., 4] = np.roll(cells[..., 4], -1, axis=0)                       # from y_n
    tmp[..., 5] = np.roll(np.roll(cells[..., 5], 1, axis=0), 1, axis=1)    # from x_w, y_s
    tmp[..., 6] = np.roll(np.roll(cells[..., 6], 1, axis=0), -1, axis=1)   # from x_e, y_s
    tmp[..., 7] = np.roll(np.roll(cells[..., 7], -1, axis=0), -1, axis=1)  # from x_e, y_n
    tmp[..., 8] = np.roll(np.roll(cells[..., 8], -1, axis=0), 1, axis=1)   # from x_w, y_n
    return tmp


def _moments(f):
    """local density and velocity, :325-347 (and :426-448, :692-714)."""
    local_density = 0.0 + f[..., 0]
    for kk in range(1, 9):
        local_density = local_density + f[..., kk]
    with np.errstate(divide="ignore", invalid="ignore"):
        u_x = (f[..., 1] + f[..., 5] + f[..., 8] - (f[..., 3] + f[..., 6] + f[..., 7])) / local_density
        u_y = (f[..., 2] + f[..., 5] + f[..., 6] - (f[..., 4] + f[..., 7] + f[..., 8])) / local_density
    return local_density, u_x, u_y


def timestep(cells, obstacles, density, accel, omega):
    """:207-214: accelerate_flow, propagate, rebound, collision.  `cells` is advanced in place and returned."""
    blocked = np.asarray(obstacles) != 0
    omega = float(omega)
    accelerate_flow(cells, blocked, density, accel)
    tmp = propagate(cells)
    # rebound :279-304 (speed 0 of a blocked cell keeps its value, which is tmp's)
    out = np.empty_like(cells)
    out[..., 0] = tmp[..., 0]
    for k, opposite in ((1, 3), (2, 4), (3, 1), (4, 2), (5, 7), (6, 8), (7, 5), (8, 6)):
        out[..., k] = tmp[..., opposite]
    # collision :306-407
    local_density, u_x, u_y = _moments(tmp)
    u_sq = u_x * u_x + u_y * u_y
    u = [None, u_x, u_y, -u_x, -u_y, u_x + u_y, -u_x + u_y, -u_x - u_y, u_x - u_y]
    d_equ = [W0 * local_density * (1.0 - u_sq / (2.0 * C_SQ))]
    for kk in range(1, 9):
        w = W1 if kk < 5 else W2
        d_equ.append(w * local_density * (1.0 + u[kk] / C_SQ
                                          + (u[kk] * u[kk]) / (2.0 * C_SQ * C_SQ)
                                          - u_sq / (2.0 * C_SQ)))
    fluid = ~blocked
    for kk in range(9):
        relaxed = tmp[..., kk] + omega * (d_equ[kk] - tmp[..., kk])
        out[..., kk][fluid] = relaxed[fluid]
    cells[...] = out
    return cells


def tot_u(cells, obstacles):
    """The sum av_velocity() divides (:409-455), and the number of cells it ran over."""
    fluid = np.asarray(obstacles) == 0
    _, u_x, u_y = _moments(cells)
    speed = np.sqrt((u_x * u_x) + (u_y * u_y))
    return float(np.sum(speed[fluid])), int(fluid.sum())


def av_velocity(cells, obstacles):
    """:409-458."""
    total, n = tot_u(cells, obstacles)
    return total / float(n)


def final_state(cells, obstacles, density):
    """write_values() :684-719: u_x, u_y, u, pressure as (ny, nx) arrays; blocked cells 0, 0, 0, density * c_sq."""
    blocked = np.asarray(obstacles) != 0
    local_density, u_x, u_y = _moments(cells)
    speed = np.sqrt((u_x * u_x) + (u_y * u_y))
    pressure = local_density * C_SQ
    return {"u_x": np.where(blocked, 0.0, u_x), "u_y": np.where(blocked, 0.0, u_y), "u": np.where(blocked, 0.0, speed),
            "pressure": np.where(blocked, float(density) * C_SQ, pressure)}


def run(cells, obstacles, density, accel, omega, n_steps):
    """The driver loop :166-170: n_steps timesteps in place; returns av_vels[n_steps]."""
    av = np.empty(n_steps, dtype=np.float64)
    for tt in range(n_steps):
        timestep(cells, obstacles, density, accel, omega)
        av[tt] = av_velocity(cells, obstacles)
    return av

"""accelerate_flow and collision for ONE cell in plain Python floats (IEEE doubles), written operation by operation from
SerialCode/d2q9-bgk.c:216-246 and :306-407 with `float` read as `double`: a second float64 reference, independent of
tests/double_model.py -- no arrays, nothing shared with it.  tests/test_double_edge_lattice.py holds the two together bit
for bit.  `timestep` strings the cell functions into the whole step (propagate :248-277, rebound :279-304) over nested lists.

Python raises on a float division by zero where C gives an infinity or a NaN: `_div` is the IEEE quotient.
"""
import math

NSPEEDS = 9


def _div(a, b):
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def accelerate_cell(speeds, density, accel):
    """:219-242 for one unblocked cell of row ny-2; returns the new nine speeds."""
    w1 = density * accel / 9.0
    w2 = density * accel / 36.0
    s = list(speeds)
    if (s[3] - w1) > 0.0 and (s[6] - w2) > 0.0 and (s[7] - w2) > 0.0:
        s[1] += w1
        s[5] += w2
        s[8] += w2
        s[3] -= w1
        s[6] -= w2
        s[7] -= w2
    return s


def collide_cell(tmp, omega):
    """:308-401 for one unblocked cell: `tmp` its nine speeds after propagate; returns the relaxed nine."""
    c_sq = 1.0 / 3.0
    w0 = 4.0 / 9.0
    w1 = 1.0 / 9.0
    w2 = 1.0 / 36.0
    local_density = 0.0
    for kk in range(NSPEEDS):
        local_density += tmp[kk]
    u_x = _div(tmp[1] + tmp[5] + tmp[8] - (tmp[3] + tmp[6] + tmp[7]), local_density)
    u_y = _div(tmp[2] + tmp[5] + tmp[6] - (tmp[4] + tmp[7] + tmp[8]), local_density)
    u_sq = u_x * u_x + u_y * u_y
    u = [0.0] * NSPEEDS
    u[1] = u_x
    u[2] = u_y
    u[3] = -u_x
    u[4] = -u_y
    u[5] = u_x + u_y
    u[6] = -u_x + u_y
    u[7] = -u_x - u_y
    u[8] = u_x - u_y
    d_equ = [0.0] * NSPEEDS
    d_equ[0] = w0 * local_density * (1.0 - u_sq / (2.0 * c_sq))
    for kk in range(1, NSPEEDS):
        w = w1 if kk <= 4 else w2
        d_equ[kk] = w * local_density * (1.0 + u[kk] / c_sq
                                         + (u[kk] * u[kk]) / (2.0 * c_sq * c_sq)
                                         - u_sq / (2.0 * c_sq))
    return [tmp[kk] + omega * (d_equ[kk] - tmp[kk]) for kk in range(NSPEEDS)]


def timestep(cells, obstacles, density, accel, omega):
    """:207-214 on cells[jj][ii] = list of nine floats, obstacles[jj][ii] = int; returns the new nested list."""
    ny, nx = len(cells), len(cells[0])
    jj = ny - 2
    cells = [[list(c) for c in row] for row in cells]
    for ii in range(nx):
        if not obstacles[jj][ii]:
            cells[jj][ii] = accelerate_cell(cells[jj][ii], density, accel)
    out = []
    for jj in range(ny):
        row = []
        for ii in range(nx):
            y_n = (jj + 1) % ny
            x_e = (ii + 1) % nx
            y_s = jj + ny - 1 if jj == 0 else jj - 1
            x_w = ii + nx - 1 if ii == 0 else ii - 1
            tmp = [cells[jj][ii][0], cells[jj][x_w][1], cells[y_s][ii][2], cells[jj][x_e][3], cells[y_n][ii][4],
                   cells[y_s][x_w][5], cells[y_s][x_e][6], cells[y_n][x_e][7], cells[y_n][x_w][8]]
            if obstacles[jj][ii]:
                # :291-298; speed 0 keeps the value `cells` holds, which propagate copied unchanged
                row.append([tmp[0], tmp[3], tmp[4], tmp[1], tmp[2], tmp[7], tmp[8], tmp[5], tmp[6]])
            else:
                row.append(collide_cell(tmp, omega))
        out.append(row)
    return out

"""The constants of ekf-slam_amd/csrc/atan2_dd.hpp: sin(k/64) and cos(k/64), k = 0..51, and π, π/2,
each as a double-double pair (hi = the nearest double, lo = the nearest double to the rest), printed
as C++ hexadecimal literals. Needs mpmath."""
import mpmath as mp

mp.mp.prec = 400


def pair(v):
    hi = float(v)
    return hi, float(v - mp.mpf(hi))


if __name__ == "__main__":
    for k in range(52):
        a = mp.mpf(k) / 64
        print("      {%s, %s, %s, %s}," % tuple(float.hex(v) for v in pair(mp.sin(a)) + pair(mp.cos(a))))
    for name, v in (("kPi", mp.pi), ("kHalfPi", mp.pi / 2)):
        print(name, ", ".join(float.hex(x) for x in pair(v)))

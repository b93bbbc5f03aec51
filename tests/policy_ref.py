"""
The device action draw (slhip_sample_actions, k_sample_actions in csrc/sl_rollout.hip) restated on the host, and the
high-precision reference it is held against.  numpy only; nothing here loads the library.

``draw_u24`` / ``sample_model`` are an EXACT model: the kernel's integer arithmetic in np.uint64 (wrapping) and its
fp32 running sum in np.float32 (IEEE adds, one rounding each, in index order), so kernel == model bit for bit.

``choice_reference`` is what the reference's host draw does (training/ppo.py:68, ``Generator.choice(n, p=probs)``:
a float64 cdf normalised by its last entry, searched with ``side="right"``) with the uniform given instead of drawn.

The contract of the draw, with ``cum_k`` the fp32 running sum over ALL A entries in index order:
    the first k with u < cum_k; if there is none, the largest k with p_k > 0; if no entry is positive, A-1.
An action with p_k == 0 is never returned while any entry is positive, and the result is in [0, A) whatever the row
holds (NaN, inf, negative entries -- their action is otherwise unspecified).
"""
import numpy as np

G = 0x9E3779B97F4A7C15          # splitmix64's increment
K = 0x100000001B3               # counter stride: z = seed + G * (counter * K + env + 1)
MASK = (1 << 64) - 1


def _u64(x):
    """Anything integer (Python ints of any size, np.uint64, signed arrays) -> np.uint64 array, reduced mod 2^64."""
    a = np.asarray(x)
    if a.dtype == np.uint64:
        return a
    if a.dtype == object or a.dtype.kind not in "iu":
        flat = [int(v) & MASK for v in np.asarray(x, dtype=object).ravel()]
        return np.array(flat, dtype=np.uint64).reshape(a.shape)
    return a.astype(np.uint64)          # signed -> two's complement, which IS reduction mod 2^64


def draw_u24(seed, counter, env_index):
    """The kernel's uniform as an integer in [0, 2^24): the top 24 bits of splitmix64's finalizer applied to
    ``seed + G * (counter * K + env_index + 1)`` (mod 2^64).  The arguments broadcast; the result is np.uint32 of the
    broadcast shape.  ``float32(u24) * 2^-24`` is exact, and is the kernel's u."""
    seed, counter, env_index = np.broadcast_arrays(_u64(seed), _u64(counter), _u64(env_index))
    shape = seed.shape
    seed, counter, env_index = (np.atleast_1d(v) for v in (seed, counter, env_index))   # (arrays wrap silently)
    z = seed + np.uint64(G) * (counter * np.uint64(K) + env_index + np.uint64(1))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.uint32).reshape(shape)


def uniform_f32(u24):
    """u = u24 * 2^-24 as float32 (exact: 24 bits fit the significand)."""
    return np.asarray(u24).astype(np.float32) * np.float32(2.0 ** -24)


def model_with_u(probs_f32, u_f32):
    """The rule of the contract for given uniforms: float32 [B, A] rows, float32 [B] uniforms -> int32 [B]."""
    p = np.asarray(probs_f32)
    if p.dtype != np.float32 or p.ndim != 2:
        raise ValueError("probs must be float32 [B, A]")
    u = np.asarray(u_f32, dtype=np.float32)
    B, A = p.shape
    cum = np.zeros(B, np.float32)
    action = np.full(B, A - 1, np.int32)
    found = np.zeros(B, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(A):
            pk = p[:, k]
            cum = cum + pk                              # float32 + float32: one IEEE rounding, like the kernel's add
            assert cum.dtype == np.float32
            action[~found & (pk > 0)] = k               # the largest positive entry so far ...
            hit = ~found & (u < cum)                    # ... until the first k with u < cum_k (strict)
            action[hit] = k
            found |= hit
    return action


def sample_model(probs_f32, seed, counter, first_env=0):
    """What ``slhip_sample_actions(probs, B, A, seed, counter, ...)`` writes, row e drawing as env ``first_env + e``
    (``first_env`` = 0 is the kernel call itself; the kernel called with ``seed + G * first_env`` gives the same)."""
    p = np.asarray(probs_f32)
    env = _u64(first_env) + np.arange(p.shape[0], dtype=np.uint64)
    return model_with_u(p, uniform_f32(draw_u24(seed, counter, env)))


def choice_reference(probs, u):
    """numpy's ``Generator.choice(A, p=probs)`` with the uniform u given: ``cdf = cumsum(p)`` in float64,
    ``cdf /= cdf[-1]``, ``searchsorted(cdf, u, side="right")``.  Rows of [B, A] against u [B]; returns (actions int64
    [B], cdf float64 [B, A]).  (side="right" on a nondecreasing row is the number of entries <= u, which is how all
    rows are searched at once.)"""
    cdf = np.cumsum(np.asarray(probs, dtype=np.float64), axis=1)
    cdf /= cdf[:, -1:]
    u = np.asarray(u, dtype=np.float64)
    return (cdf <= u[:, None]).sum(axis=1), cdf

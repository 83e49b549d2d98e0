"""The token ring restated in plain Python over bytes, for the ring tests: the
token (MurmurHash3 x86_32, seed 0), the partition key, Cluster::new's ring
(src/cluster.rs:46-54) as a dict with overwrite, replicas_for as the two loops
of src/cluster.rs:106-121 (not the library's precomputed table) and the
ownership filter of cb_tables_compact_ring. A plain module: no test, nothing
collected."""
import bisect

SEP = b"|"
M32 = 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def murmur3_32(data: bytes, seed: int = 0) -> int:
    h = seed
    c1, c2 = 0xCC9E2D51, 0x1B873593
    n = len(data)
    for i in range(0, n - n % 4, 4):
        k = int.from_bytes(data[i:i + 4], "little")
        k = (k * c1) & M32
        k = _rotl(k, 15)
        k = (k * c2) & M32
        h ^= k
        h = _rotl(h, 13)
        h = (h * 5 + 0xE6546B64) & M32
    tail = data[n - n % 4:]
    if tail:
        k = int.from_bytes(tail, "little")
        k = (k * c1) & M32
        k = _rotl(k, 15)
        k = (k * c2) & M32
        h ^= k
    h ^= n
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def partition_key(key: bytes, skip: int = 0, npk: int = 0) -> bytes:
    rest = key[min(skip, len(key)):]
    parts = rest.split(SEP)
    if npk == 0 or len(parts) <= npk:
        return rest
    return SEP.join(parts[:npk])  # parts.join("|"), src/query.rs:709,748


class Ring:
    """ring: {token: node index}, as the BTreeMap after Cluster::new."""

    def __init__(self, names=None, vnodes=8, rf=1, pairs=None, nnodes=None):
        self.ring = {}
        if pairs is None:
            self.nnodes = len(names)
            for i, name in enumerate(names):
                for v in range(max(vnodes, 1)):
                    self.ring[murmur3_32(name + b"-" + str(v).encode())] = i  # a later insert replaces
        else:
            self.nnodes = nnodes
            for t, o in pairs:
                self.ring[t] = o
        self.rf = max(rf, 1)
        self.sorted = sorted(self.ring)
        self.width = min(self.rf, len(set(self.ring.values())))

    def tokens(self):
        return self.sorted, [self.ring[t] for t in self.sorted]

    def replicas_for_token(self, token: int):
        reps = []
        for t in self.sorted[bisect.bisect_left(self.sorted, token):]:  # self.ring.range(token..)
            node = self.ring[t]
            if node not in reps:
                reps.append(node)
            if len(reps) == self.rf:
                return reps
        for t in self.sorted:
            node = self.ring[t]
            if node not in reps:
                reps.append(node)
            if len(reps) == self.rf:
                break
        return reps

    def replicas(self, key: bytes, skip=0, npk=0):
        """(token, the rf-wide list with -1 past the replicas)."""
        token = murmur3_32(partition_key(key, skip, npk))
        reps = self.replicas_for_token(token)
        return token, reps + [-1] * (self.rf - len(reps))

    def owned(self, key: bytes, node: int, rules, ranks=0) -> bool:
        """rules: [(prefix, npk)]; a key under no prefix is every node's."""
        for prefix, npk in rules:
            if key.startswith(prefix):
                reps = self.replicas(key, len(prefix), npk)[1]
                return node in reps[:ranks or self.rf]
        return True


def node_names(n):
    return [b"n%d" % i for i in range(n)]


# (names, vnodes, rf): the rings every ring test walks
RINGS = {"1x1": (node_names(1), 1, 1), "3x8": (node_names(3), 8, 2), "3 rf5": (node_names(3), 8, 5),
         "5x256": (node_names(5), 256, 3), "zeros": (node_names(4), 0, 0),
         "64x256": ([b"http://10.0.0.%d:8080" % i for i in range(64)], 256, 3)}
# (pairs, nnodes, rf): explicit tokens
TOKEN_RINGS = {"repeat": ([(100, 0), (200, 1), (100, 2), (300, 1)], 3, 2),
               "edges": ([(0, 1), (0xFFFFFFFF, 0), (0x80000000, 2)], 3, 3),
               "overwritten": ([(10, 0), (20, 1), (10, 2), (30, 2)], 3, 3)}

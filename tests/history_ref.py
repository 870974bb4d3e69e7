"""syncRevisions per object, as the Go reads (pkg/controllers/sync/history.go:36-120, pkg/controllers/util/history/
controller_history.go:91-176): dicts, real strings, Python lists. It shares nothing with kubeadmiral_amd.history's
packing: its own FNV, its own SafeEncodeString, its own ParseInt, its stable sort is ``sorted``.

``sync_revisions(obj)`` takes one entry of ``RevisionBatch.objs`` (name, wanted, limit, collision, patch, revisions,
pth, error) and returns (status, error, actions, collision, lastRevisionNameWithHash, currentRevisionName) with actions
as (kind, revision name, number)."""
import functools

ALPHABET = "bcdfghjklmnpqrstvwxz2456789"
HASH_LABEL = "controller.kubernetes.io/hash"
ZERO_TIME = -62135596800


def fnv1_32(data: bytes, h: int = 2166136261) -> int:
    for b in data:
        h = (h * 16777619) % (1 << 32)
        h ^= b
    return h


def safe_encode_string(s: str) -> str:
    return "".join(ALPHABET[ord(c) % len(ALPHABET)] for c in s)


def hash_controller_revision(raw: bytes, probe) -> str:
    """controller_history.go:93-105 (Data.Object is nil)."""
    h = fnv1_32(raw) if len(raw) > 0 else 2166136261
    if probe is not None:
        h = fnv1_32(str(int(probe)).encode(), h)
    return safe_encode_string(str(h))


def controller_revision_name(prefix: str, hash_: str) -> str:
    p = prefix.encode()
    if len(p) > 223:
        p = p[:223]
    return p.decode(errors="surrogateescape") + "-" + hash_


def parse_int_10_32(s: str):
    """strconv.ParseInt(s, 10, 32) → the int, or None on an error."""
    if s == "":
        return None
    neg, body = False, s
    if s[0] in "+-":
        neg, body = s[0] == "-", s[1:]
    if body == "":
        return None
    n = 0
    for c in body:
        if c < "0" or c > "9":
            return None
        n = n * 10 + (ord(c) - 48)
    if neg:
        n = -n
    if n < -(1 << 31) or n > (1 << 31) - 1:
        return None
    return n


def _raw(rev) -> bytes:
    d = rev.get("data")
    if d is None:
        return b""
    assert isinstance(d, (bytes, bytearray)), "the reference takes Data.Raw as bytes"
    return bytes(d)


def _labels(rev):
    return (rev.get("metadata") or {}).get("labels")


def _name(rev) -> str:
    return (rev.get("metadata") or {}).get("name") or ""


def _time(rev) -> int:
    t = (rev.get("metadata") or {}).get("creationTimestamp")
    return ZERO_TIME if t is None else t


def equal_revision(lhs, rhs_labels, rhs_raw) -> bool:
    """controller_history.go:120-143."""
    lhs_hash = rhs_hash = None
    ll = _labels(lhs) or {}
    if HASH_LABEL in ll:
        v = parse_int_10_32(ll[HASH_LABEL])
        if v is not None:
            lhs_hash = v % (1 << 32)
    if HASH_LABEL in rhs_labels:
        v = parse_int_10_32(rhs_labels[HASH_LABEL])
        if v is not None:
            rhs_hash = v % (1 << 32)
    if lhs_hash is not None and rhs_hash is not None and lhs_hash != rhs_hash:
        return False
    return _raw(lhs) == rhs_raw


def is_label_subset(x, y) -> bool:
    """sync/history.go:122-136."""
    if y is None or len(y) == 0:
        return True
    if x is None or len(x) == 0:
        return False
    for k, v in y.items():
        if x.get(k, "") != v:
            return False
    return True


def _less(a, b) -> bool:
    """byRevision.Less (controller_history.go:168-176)."""
    if a["revision"] == b["revision"]:
        if _time(a) == _time(b):
            return _name(a).encode() < _name(b).encode()
        return _time(b) > _time(a)
    return a["revision"] < b["revision"]


def _wrap(v: int) -> int:
    v %= 1 << 64
    return v - (1 << 64) if v >= 1 << 63 else v


def sync_revisions(obj):
    collision, limit = obj["collision"], obj["limit"]
    if limit == 0:
        return ("AllOK", None, [], collision, "", "")
    if obj["error"] is not None:
        return ("Error", obj["error"], [], collision, "", "")
    actions = []
    patch = obj["patch"]
    # newRevision (history.go:191-211, controller_history.go:66-89)
    hash_ = hash_controller_revision(patch, collision)
    upd_labels = dict(obj["wanted"])
    upd_labels[HASH_LABEL] = hash_
    upd_name = controller_revision_name(obj["name"], hash_)
    cur, old = [], []
    for rev in obj["revisions"]:
        (cur if equal_revision(rev, upd_labels, patch) else old).append(rev)
    mx = 0
    for rev in old:
        if rev["revision"] > mx:
            mx = rev["revision"]
    number = _wrap(mx + 1)
    if len(cur) == 0:
        actions.append(("create", upd_name, 0))
    else:
        keep = cur[0]
        for c in cur:
            if c["revision"] > keep["revision"]:
                keep = c
        for c in cur:
            if _name(c) == _name(keep):
                continue
            actions.append(("delete", _name(c), 0))
        if keep["revision"] < number:
            actions.append(("renumber", _name(keep), number))
        elif not is_label_subset(_labels(keep), obj["wanted"]):
            actions.append(("relabel", _name(keep), keep["revision"]))
    old = sorted(old, key=functools.cmp_to_key(lambda a, b: -1 if _less(a, b) else (1 if _less(b, a) else 0)))
    to_kill = _wrap(len(old) - limit)
    for rev in old:
        if to_kill <= 0:
            break
        actions.append(("delete", _name(rev), 0))
        to_kill -= 1
    last = ""
    if len(old) >= 1 and limit >= 1:
        last = _name(old[-1])
    if last != "" and obj["pth"] is not None:
        last = last + "|" + obj["pth"]
    for rev in old:
        if not is_label_subset(_labels(rev), obj["wanted"]):
            actions.append(("relabel", _name(rev), rev["revision"]))
    return ("AllOK", None, actions, collision, last, upd_name)


def outcome_tuple(o):
    """A history.RevisionOutcome in sync_revisions' shape."""
    return (o.status, o.error, list(o.actions), o.collision_count, o.last_revision_name_with_hash, o.current_revision_name)

"""Revision history for a batch of federated objects: the host half of ``kad_revision_plan``.

``SyncController.syncRevisions`` (pkg/controllers/sync/history.go:36-120, with pkg/controllers/util/history/
controller_history.go:91-176) runs per object between ensureFinalizer and ensureAnnotations: it hashes the patch of the
object's pod template, finds the listed ControllerRevisions that equal it, creates, dedups, renumbers or relabels the
current one, truncates the old ones to the history limit and relabels them. :class:`RevisionBatch` packs objects and
their listed revisions into the arrays of include/kad_sched.h (the strings stay here: names become per-object ranks,
labels interned (key, value) pairs, hash labels a flag and a number), :func:`plan_numpy` restates the device's outputs
on the CPU over the same arrays, and :meth:`RevisionBatch.apply` turns the outputs into :class:`RevisionOutcome`: the
ordered actions and the three values the reference returns. The API calls, the create-collision retry
(controller_history.go:278-320) and the events are the caller's.

Unpinned against the reference: rand.SafeEncodeString's alphabet (apimachinery is not vendored there) and
the pod template hash behind ``lastRevisionNameWithHash``'s ``|`` (HashObject goes through go-spew): the caller passes it.
"""

from __future__ import annotations

import datetime
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import gojson

HASH_LABEL = "controller.kubernetes.io/hash"  # ControllerRevisionHashLabel
ALPHANUMS = "bcdfghjklmnpqrstvwxz2456789"     # k8s.io/apimachinery/pkg/util/rand
ACT_CREATE, ACT_DELETE, ACT_RENUMBER, ACT_RELABEL = "create", "delete", "renumber", "relabel"
_KINDS = {1: ACT_CREATE, 2: ACT_DELETE, 3: ACT_RENUMBER, 4: ACT_RELABEL}
OBJ_COLLISION, OBJ_LABELS_ON_HOST = 1, 2
REV_HASH_PARSED = 1
MAX_REVISIONS = 4096
STATUS_OK, STATUS_ERROR = "AllOK", "Error"
ZERO_TIME = -62135596800  # Go's zero time.Time in Unix seconds
_PRIME, _OFFSET, _M32 = 16777619, 2166136261, 0xFFFFFFFF


class RevisionError(ValueError):
    """syncRevisions returned an error for the object."""


def safe_encode(s: str) -> str:
    """rand.SafeEncodeString: every byte b becomes ALPHANUMS[b % 27]."""
    return "".join(ALPHANUMS[b % 27] for b in s.encode())


def hash_label(sum32: int) -> str:
    """HashControllerRevision's return for the FNV sum (controller_history.go:104)."""
    return safe_encode(str(sum32))


def revision_name(prefix: str, hash_: str) -> str:
    """ControllerRevisionName (controller_history.go:53-59): the prefix cut to 223 bytes."""
    p = prefix.encode("utf-8", "surrogateescape")[:223]
    return p.decode("utf-8", "surrogateescape") + "-" + hash_


def parse_int32(s: str) -> Optional[int]:
    """strconv.ParseInt(s, 10, 32); None where Go returns an error (syntax or range)."""
    body = s[1:] if s[:1] in ("+", "-") else s
    if not body or any(c not in "0123456789" for c in body):
        return None
    v = int(body) * (-1 if s[:1] == "-" else 1)
    return v if -(1 << 31) <= v < (1 << 31) else None


def seconds(ts) -> int:
    """A creationTimestamp (RFC 3339 text, Unix seconds, or None for Go's zero time) in seconds."""
    if ts is None or ts == "":
        return ZERO_TIME
    if isinstance(ts, int):
        return ts
    t = datetime.datetime.fromisoformat(ts.replace("Z", "+00:00"))
    return int(t.timestamp()) if t.tzinfo else int(t.replace(tzinfo=datetime.timezone.utc).timestamp())


def data_raw(data) -> bytes:
    """A listed revision's Data.Raw: bytes as they are; a decoded value as FromUnstructured re-marshals it; nil empty."""
    if data is None:
        return b""
    if isinstance(data, (bytes, bytearray)):
        return bytes(data)
    return gojson.marshal_unstructured(data)


def get_patch(obj: dict) -> bytes:
    """getPatch (history.go:252-278); RevisionError without spec.template.spec.template (or a non-map on the way)."""
    v = obj
    for k in ("spec", "template", "spec", "template"):
        if not isinstance(v, dict):
            raise RevisionError("spec.template.spec.template accessor error: a value on the path is not a map")
        if k not in v:
            raise RevisionError("spec.template.spec.template is not found")
        v = v[k]
    if not isinstance(v, dict):
        raise RevisionError("spec.template.spec.template accessor error: the value is not a map")
    return gojson.revision_patch(v)


def _nested_int64(obj: dict, *path) -> int:
    v = obj
    for k in path:
        if not isinstance(v, dict) or k not in v:
            return 0
        v = v[k]
    return v if isinstance(v, int) and not isinstance(v, bool) and -(1 << 63) <= v < (1 << 63) else 0


def history_limit(obj: dict) -> int:
    """RevisionHistoryLimit (sync/resource.go:133-136)."""
    return _nested_int64(obj, "spec", "revisionHistoryLimit")


def collision_count(obj: dict) -> int:
    """CollisionCount (sync/resource.go:127-131): never nil, int32(status.collisionCount)."""
    v = _nested_int64(obj, "status", "collisionCount") & _M32
    return v - (1 << 32) if v >= (1 << 31) else v


def wanted_labels(obj: dict) -> Dict[str, str]:
    """revisionLabelsWithOriginalLabel (history.go:291-304)."""
    md = obj.get("metadata") or {}
    out = {"uid": str(md.get("uid") or "")}
    out.update(md.get("labels") or {})
    return out


def list_revisions(obj: dict, store: Sequence[dict]) -> List[dict]:
    """listRevisions / ListControllerRevisions (history.go:185-188, controller_history.go:243-276) over the store's
    ControllerRevisions, in store order: the uid label selects, the namespace is the parent's, and the controller
    owner is absent or the parent."""
    md = obj.get("metadata") or {}
    uid, ns = str(md.get("uid") or ""), md.get("namespace") or ""
    out = []
    for r in store:
        rm = r.get("metadata") or {}
        if (rm.get("labels") or {}).get("uid") != uid or (rm.get("namespace") or "") != ns:
            continue
        ref = next((o for o in rm.get("ownerReferences") or [] if o.get("controller")), None)
        if ref is None or ref.get("uid") == uid:
            out.append(r)
    return out


def label_subset(x: Optional[Dict[str, str]], y: Optional[Dict[str, str]]) -> bool:
    """IsLabelSubset (history.go:122-136): a missing key of x reads as ""."""
    if not y:
        return True
    if not x:
        return False
    return all(x.get(k, "") == v for k, v in y.items())


@dataclass
class RevisionOutcome:
    """One object's outcome of syncRevisions: ``actions`` are (kind, revision name, number) in the reference's order
    (create: the new revision's name and its Revision 0; delete: 0; renumber: the new Revision; relabel: the Revision
    UpdateControllerRevision restores), then the three return values (history.go:119)."""
    status: str = STATUS_OK
    error: Optional[str] = None
    actions: List[Tuple[str, str, int]] = field(default_factory=list)
    collision_count: Optional[int] = None
    last_revision_name_with_hash: str = ""
    current_revision_name: str = ""


class RevisionBatch:
    """Objects and their listed ControllerRevisions as kad_revision_plan's arrays."""

    def __init__(self):
        self.objs: List[dict] = []
        self._pairs: Dict[Tuple[str, str], int] = {}
        self._arrays = None

    def __len__(self):
        return len(self.objs)

    def add(self, name: str, wanted: Dict[str, str], limit: int, collision: Optional[int], patch: Optional[bytes],
            revisions: Sequence[dict], pod_template_hash: Optional[str] = None, error: Optional[str] = None) -> int:
        """One object: its name (the new revision's prefix), the wanted labels, historyLimit, the collision count
        (None: a nil pointer), the patch (None with ``error``: getPatch failed) and its listed revisions, each
        ``{"metadata": {"name", "labels", "creationTimestamp"}, "revision", "data"}``."""
        if len(revisions) > MAX_REVISIONS:
            raise ValueError(f"more than {MAX_REVISIONS} revisions on one object")
        self.objs.append(dict(name=name, wanted=dict(wanted), limit=int(limit), collision=collision, patch=patch,
                              revisions=list(revisions), pth=pod_template_hash, error=error))
        self._arrays = None
        return len(self.objs) - 1

    def _pair(self, k: str, v: str) -> int:
        return self._pairs.setdefault((k, v), len(self._pairs))

    def arrays(self) -> dict:
        """The keyword arguments of runtime.revision_plan_args / Context.revision_plan (``n_pairs`` among them)."""
        if self._arrays is not None:
            return dict(self._arrays)
        O = len(self.objs)
        limit, coll, flags = np.zeros(O, np.int64), np.zeros(O, np.int32), np.zeros(O, np.uint8)
        patch_off, patch_len = np.zeros(O, np.int64), np.zeros(O, np.int32)
        rev_off, want_off, want_lab = [0], [0], []
        d_off, d_len, revision, time_, name_rank, rflags, rhash, lab_off, lab = [], [], [], [], [], [], [], [0], []
        chunks, at = [], 0

        def put(raw: bytes) -> int:
            nonlocal at
            start = at
            pad = -len(raw) % 16
            chunks.append(raw + b"\0" * pad)
            at += len(raw) + pad
            return start

        for i, o in enumerate(self.objs):
            skip = o["error"] is not None or o["limit"] == 0
            limit[i] = 0 if skip else o["limit"]
            if o["collision"] is not None:
                coll[i], flags[i] = o["collision"], OBJ_COLLISION
            if any(v == "" for v in o["wanted"].values()):
                flags[i] |= OBJ_LABELS_ON_HOST
            patch = o["patch"] or b""
            patch_off[i], patch_len[i] = put(patch), len(patch)
            want_lab += sorted(self._pair(k, v) for k, v in o["wanted"].items())
            want_off.append(len(want_lab))
            names = [(r.get("metadata") or {}).get("name") or "" for r in o["revisions"]]
            ranks = {n: k for k, n in enumerate(sorted(set(names), key=lambda s: s.encode("utf-8", "surrogateescape")))}
            for r, nm in zip(o["revisions"], names):
                md = r.get("metadata") or {}
                labels = md.get("labels") or {}
                raw = data_raw(r.get("data"))
                d_off.append(put(raw))
                d_len.append(len(raw))
                revision.append(int(r.get("revision") or 0))
                time_.append(seconds(md.get("creationTimestamp")))
                name_rank.append(ranks[nm])
                parsed = parse_int32(labels[HASH_LABEL]) if HASH_LABEL in labels else None
                rflags.append(0 if parsed is None else REV_HASH_PARSED)
                rhash.append(0 if parsed is None else parsed & _M32)
                lab += sorted(self._pair(k, v) for k, v in labels.items())
                lab_off.append(len(lab))
            rev_off.append(len(d_off))
        blob = np.frombuffer(b"".join(chunks), np.uint8) if chunks else np.zeros(0, np.uint8)
        self._arrays = dict(
            n_pairs=len(self._pairs), limit=limit, collision=coll, obj_flags=flags, patch_off=patch_off, patch_len=patch_len,
            blob=blob, rev_off=np.array(rev_off, np.int32), rev_data_off=np.array(d_off, np.int64),
            rev_data_len=np.array(d_len, np.int32), rev_revision=np.array(revision, np.int64), rev_time=np.array(time_, np.int64),
            rev_name_rank=np.array(name_rank, np.int32), rev_flags=np.array(rflags, np.uint8), rev_hash=np.array(rhash, np.uint32),
            rev_lab_off=np.array(lab_off, np.int32), rev_lab=np.array(lab, np.int32), want_off=np.array(want_off, np.int32),
            want_lab=np.array(want_lab, np.int32))
        return dict(self._arrays)

    def apply(self, res: dict) -> List[RevisionOutcome]:
        """kad_revision_plan's outputs (or :func:`plan_numpy`'s) as one RevisionOutcome per object."""
        a = self.arrays()
        out = []
        for i, o in enumerate(self.objs):
            oc = RevisionOutcome(collision_count=o["collision"])
            out.append(oc)
            if o["limit"] == 0:
                continue
            if o["error"] is not None:
                oc.status, oc.error = STATUS_ERROR, o["error"]
                continue
            revs = o["revisions"]
            name = lambda k: (revs[k].get("metadata") or {}).get("name") or ""  # noqa: E731
            new_name = revision_name(o["name"], hash_label(int(res["hash"][i])))
            number = int(res["rev_number"][i])
            if int(a["obj_flags"][i]) & OBJ_LABELS_ON_HOST:
                lo = int(a["rev_off"][i])
                plan = _assemble(o, [bool(e) for e in res["equal"][lo:lo + len(revs)]], int(res["keep"][i]), number,
                                 [int(k) for k in res["order"][lo:lo + int(res["n_old"][i])]])
            else:
                lo = int(res["out_off"][i])
                n = int(res["n_actions"][i])
                plan = list(zip((int(k) for k in res["act_kind"][lo:lo + n]), (int(k) for k in res["act_rev"][lo:lo + n])))
            for kind, k in plan:
                if kind == 1:
                    oc.actions.append((ACT_CREATE, new_name, 0))
                elif kind == 2:
                    oc.actions.append((ACT_DELETE, name(k), 0))
                elif kind == 3:
                    oc.actions.append((ACT_RENUMBER, name(k), number))
                else:
                    oc.actions.append((ACT_RELABEL, name(k), int(revs[k].get("revision") or 0)))
            last = int(res["last"][i])
            if last >= 0:
                oc.last_revision_name_with_hash = name(last)
                if oc.last_revision_name_with_hash != "" and o["pth"] is not None:  # history.go:106-112
                    oc.last_revision_name_with_hash += "|" + o["pth"]
            oc.current_revision_name = new_name
        return out


def _assemble(o: dict, equal: List[bool], keep: int, number: int, order: List[int]) -> List[Tuple[int, int]]:
    """The action plan of an object whose label tests are the host's (KAD_REV_OBJ_LABELS_ON_HOST: a wanted label with
    an empty value equals a missing key, which pair ids cannot say), from the device's split, kept revision, revision
    number and sorted old revisions."""
    revs, want = o["revisions"], o["wanted"]
    labels = lambda k: (revs[k].get("metadata") or {}).get("labels")  # noqa: E731
    plan = []
    if keep < 0:
        plan.append((1, -1))
    else:
        kn = (revs[keep].get("metadata") or {}).get("name") or ""
        plan += [(2, k) for k, e in enumerate(equal) if e and ((revs[k].get("metadata") or {}).get("name") or "") != kn]
        if int(revs[keep].get("revision") or 0) < number:
            plan.append((3, keep))
        elif not label_subset(labels(keep), want):
            plan.append((4, keep))
    kill = _wrap64(len(order) - o["limit"])  # Go's int wraps
    plan += [(2, k) for k in order[:max(0, kill)]]
    plan += [(4, k) for k in order if not label_subset(labels(k), want)]
    return plan


# ------------------------------------------------------------------ the same arrays on the CPU
def _wrap64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def update_label(sum32: int) -> Tuple[bool, int]:
    """The update revision's hash label as EqualRevision reads it, from its characters: (ParseInt accepts it, uint32)."""
    v = parse_int32(hash_label(sum32))
    return (False, 0) if v is None else (True, v & _M32)


def fnv_numpy(blob: np.ndarray, off: np.ndarray, length: np.ndarray) -> np.ndarray:
    """FNV-1 32 of blob[off[i] : off[i] + length[i]] for every i: one numpy step per byte position over the strings
    that reach it (sorted by length, so they are a prefix)."""
    order = np.argsort(-length.astype(np.int64), kind="stable")
    off_s, len_s = off[order].astype(np.int64), length[order].astype(np.int64)
    h = np.full(len(order), _OFFSET, np.uint64)
    for t in range(int(len_s[0]) if len(len_s) else 0):
        n = int(np.searchsorted(-len_s, -t, side="left"))  # the strings longer than t
        h[:n] = ((h[:n] * _PRIME) & _M32) ^ blob[off_s[:n] + t]
    out = np.zeros(len(order), np.uint32)
    out[order] = h.astype(np.uint32)
    return out


def plan_numpy(n_pairs: int, **a) -> dict:
    """kad_revision_plan's outputs from its input arrays, on the CPU."""
    O, R = len(a["obj_flags"]), len(a["rev_flags"])
    rev_off, blob = a["rev_off"], a["blob"]
    live = a["limit"] != 0
    h = fnv_numpy(blob, a["patch_off"], np.where(live, a["patch_len"], 0))
    out_off = np.zeros(O + 1, np.int64)
    out_off[1:] = np.cumsum(2 * np.diff(rev_off).astype(np.int64) + 1)
    res = dict(out_off=out_off, hash=np.zeros(O, np.uint32), upd_hash=np.zeros(O, np.uint32), upd_parsed=np.zeros(O, np.uint8),
               equal=np.zeros(R, np.uint8), order=np.zeros(R, np.int32), n_old=np.zeros(O, np.int32), keep=np.full(O, -1, np.int32),
               n_actions=np.zeros(O, np.int32), last=np.full(O, -1, np.int32), rev_number=np.zeros(O, np.int64),
               act_kind=np.zeros(int(out_off[-1]), np.uint8), act_rev=np.zeros(int(out_off[-1]), np.int32))
    raw = blob.tobytes()
    for i in range(O):
        if not live[i]:
            continue
        s = int(h[i])
        if a["obj_flags"][i] & OBJ_COLLISION:
            for ch in str(int(a["collision"][i])).encode():
                s = ((s * _PRIME) & _M32) ^ ch
        parsed, val = update_label(s)
        res["hash"][i], res["upd_hash"][i], res["upd_parsed"][i] = s, val, parsed
        lo, hi = int(rev_off[i]), int(rev_off[i + 1])
        po, pl = int(a["patch_off"][i]), int(a["patch_len"][i])
        patch = raw[po:po + pl]
        want = a["want_lab"][a["want_off"][i]:a["want_off"][i + 1]].tolist()
        on_host = bool(a["obj_flags"][i] & OBJ_LABELS_ON_HOST)

        def subset(r):
            if not want:
                return True
            have = a["rev_lab"][a["rev_lab_off"][r]:a["rev_lab_off"][r + 1]].tolist()
            return bool(have) and set(want) <= set(have)

        cur, old = [], []
        for r in range(lo, hi):
            eq = int(a["rev_data_len"][r]) == pl
            if eq and (a["rev_flags"][r] & REV_HASH_PARSED) and parsed and int(a["rev_hash"][r]) != val:
                eq = False
            if eq:
                do = int(a["rev_data_off"][r])
                eq = raw[do:do + pl] == patch
            res["equal"][r] = eq
            (cur if eq else old).append(r)
        revn = a["rev_revision"]
        number = _wrap64(max([0] + [int(revn[r]) for r in old]) + 1)
        acts = []
        if not cur:
            acts.append((1, -1))
        else:
            keep = cur[0]
            for r in cur:
                if revn[r] > revn[keep]:
                    keep = r
            acts += [(2, r - lo) for r in cur if a["rev_name_rank"][r] != a["rev_name_rank"][keep]]
            if revn[keep] < number:
                acts.append((3, keep - lo))
            elif not on_host and not subset(keep):
                acts.append((4, keep - lo))
            res["keep"][i] = keep - lo
        old.sort(key=lambda r: (int(revn[r]), int(a["rev_time"][r]), int(a["rev_name_rank"][r]), r))
        limit = int(a["limit"][i])
        kill = min(len(old), max(0, _wrap64(len(old) - limit)))
        acts += [(2, r - lo) for r in old[:kill]]
        if not on_host:
            acts += [(4, r - lo) for r in old if not subset(r)]
        res["order"][lo:lo + len(old)] = [r - lo for r in old]
        res["n_old"][i], res["rev_number"][i], res["n_actions"][i] = len(old), number, len(acts)
        if old and limit >= 1:
            res["last"][i] = old[-1] - lo
        at = int(out_off[i])
        for k, (kind, r) in enumerate(acts):
            res["act_kind"][at + k], res["act_rev"][at + k] = kind, r
    return res


def batch_of(objs: Sequence[dict], revisions: Sequence[Sequence[dict]],
             pod_template_hashes: Optional[Sequence[Optional[str]]] = None) -> RevisionBatch:
    """A RevisionBatch of federated objects and, per object, its listed revisions (list_revisions' result)."""
    batch = RevisionBatch()
    for i, (obj, revs) in enumerate(zip(objs, revisions)):
        md = obj.get("metadata") or {}
        limit = history_limit(obj)
        patch, err = None, None
        if limit != 0:
            try:
                patch = get_patch(obj)
            except RevisionError as e:
                err = str(e)
        batch.add(md.get("name") or "", wanted_labels(obj), limit, collision_count(obj), patch, revs,
                  pod_template_hashes[i] if pod_template_hashes else None, err)
    return batch

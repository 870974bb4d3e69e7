"""Hand-written syncRevisions cases: name → (the object as an entry of RevisionBatch.objs, the expected actions, the
expected lastRevisionNameWithHash). ``NEW`` in an expected action stands for the update revision's name (the
object's currentRevisionName), which test_history_host.py pins separately against a hand-computed FNV sum."""
import history_ref as R

NEW = "<new>"
HL = R.HASH_LABEL
W = {"uid": "u1", "app": "web"}
P = b'[{"op":"replace","path":"/spec/template/spec/template","value":{"spec":{"containers":[{"image":"a:1"}]}}}]'
Q = P.replace(b"a:1", b"a:0")


def rev(name, revision, data, labels=W, t=0, hash_=None):
    lab = None if labels is None else dict(labels)
    if hash_ is not None:
        lab = dict(lab or {})
        lab[HL] = hash_
    return {"metadata": {"name": name, "labels": lab, "creationTimestamp": t}, "revision": revision, "data": data}


def obj(revisions, patch=P, limit=10, collision=0, wanted=W, name="web", pth=None, error=None):
    return dict(name=name, wanted=dict(wanted), limit=limit, collision=collision, patch=patch, revisions=list(revisions),
                pth=pth, error=error)


def numeric_patch():
    """The first patch of a fixed family whose update revision's hash label is all digits and fits int32: its FNV sum's
    decimal holds no digit above 5 and, every digit raised by 4, stays below 2^31 (about one sum in 400)."""
    for k in range(100000):
        p = b'[{"op":"replace","path":"/spec/template/spec/template","value":{"n":%d}}]' % k
        label = R.hash_controller_revision(p, 0)
        if R.parse_int_10_32(label) is not None:
            return p, label
    raise AssertionError("no numeric label in the family")


def pattern(n, salt=0):
    return bytes((i * 7 + salt) % 251 for i in range(n))


def flip(b, i):
    return b[:i] + bytes([b[i] ^ 0x20]) + b[i + 1:]


DATA_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 4097)


def data_case(n):
    """A patch of n bytes against: the same bytes, one byte longer, the first byte different, the last byte different."""
    p = pattern(n)
    revs = [rev("same", 100, p), rev("longer", 1, p + b"x")]
    want_last = "longer"
    if n:
        revs += [rev("first", 2, flip(p, 0)), rev("last", 3, flip(p, n - 1))]
        want_last = "last"
    return obj(revs, patch=p), [], want_last


def named():
    NP, NL = numeric_patch()
    other = str(int(NL) + 1)
    three = [rev("o1", 1, Q), rev("o2", 2, Q), rev("o3", 3, Q)]
    c = {
        "no_revisions": (obj([]), [("create", NEW, 0)], ""),
        "one_current": (obj([rev("r1", 1, P)]), [], ""),
        "one_old": (obj([rev("r1", 1, Q)]), [("create", NEW, 0)], "r1"),
        "one_old_one_current": (obj([rev("r1", 1, Q), rev("r2", 2, P)]), [], "r1"),
        "two_currents_different_revision": (obj([rev("r1", 1, P), rev("r2", 3, P)]), [("delete", "r1", 0)], ""),
        "two_currents_equal_revision": (obj([rev("r1", 2, P), rev("r2", 2, P)]), [("delete", "r2", 0)], ""),
        "three_currents_one_named_as_the_kept": (obj([rev("r1", 5, P), rev("r1", 2, P), rev("r3", 1, P)]), [("delete", "r3", 0)], ""),
        "keep_below_number": (obj([rev("c", 1, P), rev("o", 4, Q)]), [("renumber", "c", 5)], "o"),
        "keep_equal_number_relabels": (obj([rev("c", 5, P, {"uid": "u1"}), rev("o", 4, Q)]), [("relabel", "c", 5)], "o"),
        "keep_above_number": (obj([rev("c", 9, P), rev("o", 4, Q)]), [], "o"),
        "old_ties_by_time_then_name": (obj([rev("b", 3, Q, t=5), rev("a", 3, Q, t=5), rev("z", 3, Q, t=4), rev("y", 2, Q, t=9)], limit=2),
                                       [("create", NEW, 0), ("delete", "y", 0), ("delete", "z", 0)], "b"),
        "old_equal_keys_keep_list_order": (obj([rev("n", 3, Q, {"uid": "u1"}, t=5), rev("n", 3, Q, t=5), rev("n", 3, Q, None, t=5)], limit=1),
                                           [("create", NEW, 0), ("delete", "n", 0), ("delete", "n", 0), ("relabel", "n", 3), ("relabel", "n", 3)], "n"),
        "limit_1": (obj(three, limit=1), [("create", NEW, 0), ("delete", "o1", 0), ("delete", "o2", 0)], "o3"),
        "limit_equal_to_old": (obj(three, limit=3), [("create", NEW, 0)], "o3"),
        "limit_above_old": (obj(three, limit=4), [("create", NEW, 0)], "o3"),
        "limit_negative": (obj(three, limit=-1), [("create", NEW, 0), ("delete", "o1", 0), ("delete", "o2", 0), ("delete", "o3", 0)], ""),
        "limit_most_negative_wraps": (obj(three, limit=-(1 << 63)), [("create", NEW, 0)], ""),
        "limit_0": (obj(three, limit=0), [], ""),
        "limit_0_without_template": (obj(three, limit=0, patch=None, error="spec.template.spec.template is not found"), [], ""),
        "all_old_negative": (obj([rev("c", 0, P), rev("o1", -5, Q), rev("o2", -3, Q)]), [("renumber", "c", 1)], "o2"),
        "revision_number_wraps": (obj([rev("c", 7, P, {"uid": "u1"}), rev("o", (1 << 63) - 1, Q)]), [("relabel", "c", 7)], "o"),
        "collision_nil": (obj([], collision=None), [("create", NEW, 0)], ""),
        "collision_0": (obj([], collision=0), [("create", NEW, 0)], ""),
        "collision_negative": (obj([], collision=-12), [("create", NEW, 0)], ""),
        "collision_min": (obj([], collision=-(1 << 31)), [("create", NEW, 0)], ""),
        "labels_numeric_equal": (obj([rev("r", 1, NP, hash_=NL)], patch=NP), [], ""),
        "labels_numeric_different_same_bytes": (obj([rev("r", 1, NP, hash_=other)], patch=NP), [("create", NEW, 0)], "r"),
        "label_negative_number_same_bytes": (obj([rev("r", 1, NP, hash_="-1")], patch=NP), [("create", NEW, 0)], "r"),
        "label_plus_sign_equal": (obj([rev("r", 1, NP, hash_="+" + NL)], patch=NP), [], ""),
        "label_overflows_int32_same_bytes": (obj([rev("r", 1, NP, hash_="2147483648")], patch=NP), [], ""),
        "label_not_a_number_same_bytes": (obj([rev("r", 1, NP, hash_="4x")], patch=NP), [], ""),
        "label_empty_same_bytes": (obj([rev("r", 1, NP, hash_="")], patch=NP), [], ""),
        "update_label_not_numeric": (obj([rev("r", 1, P, hash_="123")]), [], ""),
        "subset_true_false_none": (obj([rev("c", 9, P), rev("ok", 1, Q, {"uid": "u1", "app": "web", "x": "y"}), rev("bad", 2, Q, {"uid": "u1", "app": "api"}),
                                        rev("none", 3, Q, None), rev("empty", 4, Q, {})]),
                                   [("relabel", "bad", 2), ("relabel", "none", 3), ("relabel", "empty", 4)], "empty"),
        "wanted_empty_value_on_host": (obj([rev("c", 9, P, {"uid": "u1"}), rev("missing", 1, Q, {"uid": "u1"}), rev("set", 2, Q, {"uid": "u1", "opt": "x"}),
                                            rev("none", 3, Q, None), rev("blank", 4, Q, {"uid": "u1", "opt": ""})], wanted={"uid": "u1", "opt": ""}),
                                       [("relabel", "set", 2), ("relabel", "none", 3)], "blank"),
        "wanted_empty_value_keep_relabel": (obj([rev("c", 9, P, {"uid": "u1", "opt": "x"})], wanted={"uid": "u1", "opt": ""}), [("relabel", "c", 9)], ""),
        "pod_template_hash_suffix": (obj([rev("o", 1, Q)], pth="5d4f"), [("create", NEW, 0)], "o|5d4f"),
        "pod_template_hash_without_last": (obj([rev("o", 1, Q)], limit=-1, pth="5d4f"), [("create", NEW, 0), ("delete", "o", 0)], ""),
        "missing_template": (obj(three, patch=None, error="spec.template.spec.template is not found"), None, ""),
        "long_name_prefix": (obj([], name="n" * 300), [("create", NEW, 0)], ""),
    }
    for n in DATA_LENGTHS:
        c[f"data_{n}"] = data_case(n)
    return c


def random_objs(seed, n, max_revs=8):
    """Seeded adversarial objects: few distinct data strings, Revisions, times, names and labels, so that ties, duplicate
    names, several current revisions and every limit meet; a tenth use the numeric-label patch with numeric labels."""
    import random
    rnd = random.Random(seed)
    NP, NL = numeric_patch()
    label_sets = [W, {"uid": "u1"}, {"uid": "u1", "app": "api"}, None, {}, {"uid": "u1", "app": "web", "extra": "1"}]
    out = []
    for i in range(n):
        numeric = rnd.random() < 0.1
        patch = NP if numeric else P
        datas = [patch, patch, Q, patch[:-1], flip(patch, len(patch) - 1), b""]
        revs = []
        for k in range(rnd.randrange(max_revs + 1)):
            h = rnd.choice([None, NL, str(int(NL) + 1), "2147483648", "zz"]) if numeric else rnd.choice([None, "77", "bcd"])
            revs.append(rev(rnd.choice("abcd"), rnd.choice([-2, 0, 1, 2, 2, 3, 7]), rnd.choice(datas), rnd.choice(label_sets),
                            t=rnd.choice([0, 5, 5, 9]), hash_=h))
        wanted = W if rnd.random() < 0.85 else {"uid": "u1", "opt": ""}
        out.append(obj(revs, patch=patch, limit=rnd.choice([-1, 0, 1, 2, 3, 10]), collision=rnd.choice([None, 0, 1, -3, 2147483647]),
                       wanted=wanted, name=f"obj-{i}", pth=rnd.choice([None, "abc"])))
    return out


def sized_obj(n_revs, seed=0, limit=3):
    """One object with exactly n_revs listed revisions: every seventh current, Revisions and times with ties, a third
    without the wanted labels."""
    revs = []
    for k in range(n_revs):
        j = (k * 2654435761 + seed) % 1000003
        revs.append(rev(f"r{j % 97}", j % 11, P if k % 7 == 3 else Q, W if j % 3 else {"uid": "u1"}, t=j % 5))
    return obj(revs, limit=limit, name=f"sized-{n_revs}")


def batch_of_entries(entries):
    from kubeadmiral_amd import history as H
    b = H.RevisionBatch()
    for e in entries:
        b.add(e["name"], e["wanted"], e["limit"], e["collision"], e["patch"], e["revisions"], e["pth"], e["error"])
    return b

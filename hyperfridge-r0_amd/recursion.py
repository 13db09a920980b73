"""lift + join tree over segment receipts: the exchange schedule of BASELINE.json configs[4].

risc0-zkvm `ProverServer::lift(SegmentReceipt)` turns every segment seal into a recursion-circuit proof, `join(a, b)` folds two of
them into one, and the folds form a binary tree whose levels are the only inter-GPU exchange of the whole path.  The proving side --
lift, join, the composition of claims ({pre: a.pre, post: b.post, ..}), the refusal of two nodes that do not follow one another --
lives in the library behind the C ABI (csrc/recursion.cpp: r0h_recursor_new / r0h_lift / r0h_join / r0h_node_*; what a node's
proof is and is not -- the digest of what it consumed computed in-circuit, the children's seals checked BESIDE the proof, not risc0's
recursion circuit -- is stated there and in include/r0hip.h).
This module is the transport only: which rank hands its subtree to which, and how a node travels.

Transport: `torch.distributed` point-to-point send/recv (backend "nccl" = RCCL over xGMI on a GPU node, "gloo" on CPU), one
process per GPU; partner of rank r at level l is r ^ (1 << l), the lower rank of a pair joins.  No collective is involved.
A node travels as its claim (the 144 bytes of r0h_receipt_claim) followed by its seal (`to_words`), or -- when its leaves' session
parts are to reach the root (r0h_root_verify_session_*) -- in wire form (`to_wire`): claim words, [n_leaves, seal_words], seal,
session words.
"""
import ctypes

import numpy as np

from . import Hal, NODE_SESSION_WORDS, ReceiptClaim, R0HipError, _check, _u32arr, _vp, _sz, lib, seal_digest, verify_seal  # noqa: F401  (package __init__ is the ctypes harness)

RECURSION_PO2 = 18
CLAIM_WORDS = ctypes.sizeof(ReceiptClaim) // 4


def tree_schedule(world):
    """[(level, receiver, sender), ...] of the binary join tree over ranks 0..world-1 (any world size >= 1)."""
    plan, stride = [], 1
    while stride < world:
        for r in range(0, world, 2 * stride):
            if r + stride < world:
                plan.append((stride.bit_length() - 1, r, r + stride))
        stride *= 2
    return plan


class Node:
    """A proven tree node (r0h_node): its seal, the composed claim it is carried with and `session`, its leaves' session parts in leaf
    order as an (n, 48) array (n = 0: a leaf below it is no trace-circuit segment, or the node arrived without them)."""

    def __init__(self, handle):
        self.handle = handle
        p, n = _vp(), _sz(0)
        _check(lib().r0h_node_seal(handle, ctypes.byref(p), ctypes.byref(n)))
        self.seal = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint32)), shape=(n.value,)).copy()
        self.claim = ReceiptClaim()
        _check(lib().r0h_node_claim(handle, ctypes.byref(self.claim)))
        p, n = _vp(), _sz(0)
        _check(lib().r0h_node_session(handle, ctypes.byref(p), ctypes.byref(n)))
        self.session = np.zeros((0, NODE_SESSION_WORDS), dtype=np.uint32)
        if n.value:
            self.session = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint32)), shape=(n.value, NODE_SESSION_WORDS)).copy()

    @classmethod
    def from_parts(cls, seal, claim, session=None):
        a, pa = _u32arr(seal)
        h = _vp()
        if session is None:
            _check(lib().r0h_node_new(pa, a.size, ctypes.byref(claim), ctypes.byref(h)))
        else:
            b, pb = _u32arr(np.asarray(session, dtype=np.uint32).reshape(-1, NODE_SESSION_WORDS))
            _check(lib().r0h_node_new_with_session(pa, a.size, ctypes.byref(claim), pb, b.shape[0], ctypes.byref(h)))
        return cls(h)

    def to_wire(self):
        """claim words, [n_leaves, seal_words], seal, session words"""
        head = np.array([self.session.shape[0], self.seal.size], dtype=np.uint32)
        return np.concatenate([np.frombuffer(bytes(self.claim), dtype=np.uint32), head, self.seal, self.session.reshape(-1)]).astype(np.uint32)

    @classmethod
    def from_wire(cls, words):
        words = np.ascontiguousarray(words, dtype=np.uint32)
        if words.size < CLAIM_WORDS + 2:
            raise R0HipError("a node in wire form starts with %d claim words and two counts; got %d words" % (CLAIM_WORDS, words.size))
        n_leaves, seal_words = int(words[CLAIM_WORDS]), int(words[CLAIM_WORDS + 1])
        want = CLAIM_WORDS + 2 + seal_words + n_leaves * NODE_SESSION_WORDS
        if seal_words == 0 or words.size != want:
            raise R0HipError("a node in wire form with %d leaves and a seal of %d words has %d words; got %d" % (n_leaves, seal_words, want, words.size))
        claim = ReceiptClaim.from_buffer_copy(words[:CLAIM_WORDS].tobytes())
        at = CLAIM_WORDS + 2
        return cls.from_parts(words[at:at + seal_words], claim, words[at + seal_words:] if n_leaves else None)

    def to_words(self):
        return np.concatenate([np.frombuffer(bytes(self.claim), dtype=np.uint32), self.seal]).astype(np.uint32)

    @classmethod
    def from_words(cls, words):
        words = np.ascontiguousarray(words, dtype=np.uint32)
        if words.size <= CLAIM_WORDS:
            raise R0HipError("a node on the wire is %d claim words followed by its seal; got %d words" % (CLAIM_WORDS, words.size))
        claim = ReceiptClaim.from_buffer_copy(words[:CLAIM_WORDS].tobytes())
        return cls.from_parts(words[CLAIM_WORDS:], claim)

    @property
    def digest(self):
        return seal_digest(self.seal)

    @property
    def claim_words(self):
        """public inputs 0..7: the words naming the node's composed claim"""
        return self.seal[:8].copy()

    @property
    def consumed_digest(self):
        """public inputs 8..15: the Poseidon2 digest of what the node consumed (a segment seal, or its two children's digests)"""
        return self.seal[8:16].copy()

    def free(self):
        if self.handle:
            lib().r0h_node_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Recursor:
    """lift / join on one device (r0h_recursor).  `segment_blob` is the circuit the leaf seals belong to; `segment_roots`
    {po2: root[8]} binds the leaves to the segment program (without it they are verified against the circuit alone)."""

    def __init__(self, hal, recursion_blob, segment_blob, code_object=None, po2=RECURSION_PO2, segment_roots=None):
        self.hal, self.po2 = hal, po2
        self.recursion_blob = np.ascontiguousarray(recursion_blob, dtype=np.uint32)
        rb, prb = _u32arr(self.recursion_blob)
        sb, psb = _u32arr(segment_blob)
        roots = np.zeros(9 * max(len(segment_roots or {}), 1), dtype=np.uint32)
        for k, (size, root) in enumerate(sorted((segment_roots or {}).items())):
            roots[9 * k] = size
            roots[9 * k + 1:9 * k + 9] = root
        self.handle = _vp()
        _check(lib().r0h_recursor_new(hal.ctx, prb, rb.size, code_object.encode() if code_object else None, po2, psb, sb.size, roots.ctypes.data_as(_vp),
                                      len(segment_roots or {}), ctypes.byref(self.handle)))
        self.control_root = np.zeros(8, dtype=np.uint32)
        _check(lib().r0h_recursor_control_root(self.handle, self.control_root.ctypes.data_as(_vp)))

    def set_verify_on_device(self, on=True):
        """lift / join / compress verify the seals they consume as one batch with the lane's device hashing their Merkle openings
        (r0h_recursor_set_verify_on_device), instead of on host threads beside the proof.  Off by default; refusals, messages and
        nodes are the same either way."""
        _check(lib().r0h_recursor_set_verify_on_device(self.handle, 1 if on else 0))

    def lift(self, segment_seal, claim):
        """risc0 `lift`: one recursion-circuit proof standing for one segment seal and its claim."""
        a, pa = _u32arr(segment_seal)
        h = _vp()
        _check(lib().r0h_lift(self.handle, pa, a.size, ctypes.byref(claim), ctypes.byref(h)))
        return Node(h)

    def join(self, a, b):
        """risc0 `join`: one proof standing for two nodes that follow one another; its claim is their composition."""
        h = _vp()
        _check(lib().r0h_join(self.handle, a.handle, b.handle, ctypes.byref(h)))
        return Node(h)

    def node_from_words(self, words):
        return Node.from_words(words)

    def node_from_wire(self, words):
        return Node.from_wire(words)

    def compress(self, receipt, lanes=0):
        """risc0 `prover.compress`: every segment of a composite receipt lifted and the nodes joined into one root, on `lanes` prover
        lanes (1..4; 0: 2) of this device (r0h_compress).  The root is `fold` of the lifted segments, word for word."""
        h = _vp()
        _check(lib().r0h_compress(self.handle, receipt.handle, lanes, ctypes.byref(h)))
        return Node(h)

    @staticmethod
    def verify_session(node, trace_blob, journal, elf=None, image_id=None, image_blob=None, image_proof=None, image_control_root=None):
        """A root held to what `receipt.verify` holds a receipt to beyond its seals (r0h_root_verify_session_elf, or _image with
        image_id + image_blob + image_proof): -> (verdict, reason, leaf).  Host only; `verify` checks the node's own seal."""
        b, pb = _u32arr(trace_blob)
        journal = bytes(journal)
        verdict, leaf = ctypes.c_int(-1), _sz(0)
        if elf is not None:
            elf = bytes(elf)
            _check(lib().r0h_root_verify_session_elf(pb, b.size, node.handle, journal, len(journal), elf, len(elf), ctypes.byref(verdict), ctypes.byref(leaf)))
        else:
            ib, pib = _u32arr(image_blob)
            sl, psl = _u32arr(image_proof if image_proof is not None else np.zeros(0, dtype=np.uint32))
            proot = None
            if image_control_root is not None:
                root, proot = _u32arr(image_control_root)
            _check(lib().r0h_root_verify_session_image(pb, b.size, node.handle, journal, len(journal), pib, ib.size, proot, psl, sl.size, bytes(image_id),
                                                       ctypes.byref(verdict), ctypes.byref(leaf)))
        return verdict.value, lib().r0h_receipt_verify_reason(verdict.value).decode(), leaf.value

    def verify(self, node):
        """the node's seal verifies bound to the recursion circuit's control root and names the claim it is carried with"""
        ok = ctypes.c_int(0)
        rb, prb = _u32arr(self.recursion_blob)
        _check(lib().r0h_node_verify(prb, rb.size, self.control_root.ctypes.data_as(_vp), node.handle, ctypes.byref(ok)))
        return bool(ok.value)

    def fold(self, nodes):
        """Left-to-right binary fold of this rank's own nodes (log depth); neighbours are joined, so consecutive segments stay consecutive."""
        nodes = list(nodes)
        while len(nodes) > 1:
            nxt = [self.join(nodes[i], nodes[i + 1]) for i in range(0, len(nodes) - 1, 2)]
            if len(nodes) & 1:
                nxt.append(nodes[-1])
            nodes = nxt
        return nodes[0]

    def close(self):
        if self.handle:
            _check(lib().r0h_recursor_free(self.handle))
            self.handle = None


FAILED = np.array([0xFFFFFFFF], dtype=np.uint32)  # handed up instead of a seal by a rank whose subtree could not be proved
EMPTY = np.zeros(0, dtype=np.uint32)               # handed up by a rank that owns no segment (segments < world)


def join_across_ranks(recursor, node, rank, world, send, recv, with_session=False):
    """Run the cross-rank part of the tree.  `send(array, dst)` / `recv(src) -> array` move one node (uint32 words: claim, seal; with
    `with_session` the wire form, so that the leaves' session parts reach the root in leaf order).
    A rank's own nodes cover a contiguous run of segments and rank r's run precedes rank r + 1's (driver.shard_contiguous), so the
    receiver's node is always the LEFT operand of the join.
    Returns the root Node on rank 0 and None elsewhere.

    Every rank takes part in every exchange the schedule gives it, whatever happened before: a rank without a node (empty
    share) hands up an empty message and its partner keeps what it has; a rank whose join failed (or whose child reported a
    failure) hands up a failure marker instead of blocking its partner, so the failure reaches the root, every rank leaves
    the tree, and the first error is re-raised on the rank where it happened (and as "a child rank failed" above it)."""
    failed = None
    for _level, receiver, sender in tree_schedule(world):
        if rank == sender:
            send(FAILED if failed is not None else (EMPTY if node is None else (node.to_wire() if with_session else node.to_words())), receiver)
            if failed is not None:
                raise failed
            return None  # this rank's subtree has been handed up
        if rank == receiver:
            other = recv(sender)
            if other.size == 1 and other[0] == FAILED[0]:
                failed = failed or R0HipError("join tree: rank %d reported a failure in its subtree" % sender)
            elif failed is None and other.size:
                try:
                    arrived = recursor.node_from_wire(other) if with_session else recursor.node_from_words(other)
                    node = arrived if node is None else recursor.join(node, arrived)
                except Exception as exc:  # noqa: BLE001 -- carried up the tree, re-raised below
                    failed = exc
    if failed is not None:
        raise failed
    return node if rank == 0 else None


def torch_transport(device=None):
    """send/recv over torch.distributed point-to-point (RCCL when the process group is "nccl", gloo otherwise)."""
    import torch
    import torch.distributed as dist

    on_gpu = dist.get_backend() == "nccl"
    dev = device if on_gpu else "cpu"

    def send(words, dst):
        n = torch.tensor([int(words.size)], dtype=torch.int64, device=dev)
        dist.send(n, dst)
        if words.size:  # an EMPTY message is its length word alone: no zero-byte point-to-point transfer (both sides skip it)
            dist.send(torch.from_numpy(words.view(np.int32).copy()).to(dev), dst)

    def recv(src):
        n = torch.zeros(1, dtype=torch.int64, device=dev)
        dist.recv(n, src)
        if int(n.item()) == 0:
            return np.zeros(0, dtype=np.uint32)
        buf = torch.empty(int(n.item()), dtype=torch.int32, device=dev)
        dist.recv(buf, src)
        return buf.cpu().numpy().view(np.uint32)

    return send, recv

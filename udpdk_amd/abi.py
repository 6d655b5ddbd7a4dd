"""ctypes bindings to libudpdk_amd.so (the C ABI of include/udpdk_gpu.h and include/udpdk_api.h).

Used by tests/ and bench.py. Everything that computes goes through the shared library; numpy
arrays are only host staging for the C-ABI calls.
"""
from __future__ import annotations

import ctypes as C
import errno
import os
import socket
import struct
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UDPDK_LIB_OVERRIDE") or os.path.join(_HERE, "libudpdk_amd.so")

# ---- constants mirrored from include/udpdk_gpu.h -------------------------------------------
V_DELIVERED, V_NOT_IPV4, V_FRAG, V_NOT_UDP, V_NO_BIND, V_NO_MATCH, V_TRUNC, V_BAD_DESC = range(8)
VERDICT_NAMES = ["DELIVERED", "NOT_IPV4", "FRAG", "NOT_UDP", "NO_BIND", "NO_MATCH", "TRUNC",
                 "BAD_DESC"]
UDP_NONE, UDP_OK, UDP_BAD = 0, 1, 2
N_COUNTERS = 16
N_KERNEL_IDS = 5          # udpdk_gpu_kernel_id: classify, scan, scatter, tx_build, rx_gather
C_DELIVERIES, C_IP_BAD, C_UDP_OK, C_UDP_BAD, C_UDP_NONE, C_LEN_BAD, C_IHL_NE5, C_BYTES = range(8, 16)
K_RX_CLASSIFY, K_RX_SCAN, K_RX_SCATTER, K_TX_BUILD = range(4)
MAX_LANES = 16384


def meta_verdict(m):
    return np.asarray(m) & 0xF


def meta_sockfd(m):
    return np.asarray(m) >> 16


def meta_fanout(m):
    return (np.asarray(m) >> 9) & 0x7F


def meta_udp(m):
    return (np.asarray(m) >> 5) & 3


class Binding(C.Structure):
    _fields_ = [("ip", C.c_uint32), ("sockfd", C.c_int32), ("reuse", C.c_uint32)]


class Slot(C.Structure):
    _fields_ = [("ip", C.c_uint32), ("udp_port", C.c_uint32), ("bound", C.c_uint32)]


class BindSnapshot(C.Structure):
    _fields_ = [("port_first", C.POINTER(C.c_uint32)), ("port_count", C.POINTER(C.c_uint16)),
                ("binds", C.POINTER(Binding)), ("n_binds", C.c_uint32),
                ("n_lanes", C.c_uint32), ("lane_mask", C.c_uint32),
                ("slots", C.POINTER(Slot)), ("n_slots", C.c_uint32),
                ("version", C.c_uint64)]


class RxBatch(C.Structure):
    _fields_ = [("frames_dev", C.c_void_p), ("frames_bytes", C.c_uint64),
                ("offset_dev", C.c_void_p), ("length_dev", C.c_void_p),
                ("ptype_dev", C.c_void_p), ("n", C.c_uint32)]


class RxOut(C.Structure):
    _fields_ = [("meta_dev", C.c_void_p), ("lane_off_dev", C.c_void_p),
                ("lane_pkt_dev", C.c_void_p), ("lane_cap", C.c_uint32)]


class RxStats(C.Structure):
    _fields_ = [("counters", C.c_uint64 * N_COUNTERS), ("deliveries", C.c_uint32),
                ("overflow", C.c_uint32)]


# UDPDK_RX_DROP_*: the deliveries the RX drop filter removes
RX_DROP_IP_CKSUM, RX_DROP_UDP_CKSUM, RX_DROP_UDP_LEN, RX_DROP_IHL, RX_DROP_ALL = 1, 2, 4, 8, 15


class RxLanes(C.Structure):
    _fields_ = [("meta_dev", C.c_void_p), ("n", C.c_uint32), ("lane_off_dev", C.c_void_p),
                ("lane_pkt_dev", C.c_void_p), ("lane_cap", C.c_uint32), ("n_lanes", C.c_uint32)]


class RxDropStats(C.Structure):
    _fields_ = [("dropped", C.c_uint64 * 4), ("kept", C.c_uint32), ("removed", C.c_uint32),
                ("bad_index", C.c_uint32), ("truncated", C.c_uint32)]


class RxBalanceStats(C.Structure):
    _fields_ = [("kept", C.c_uint32), ("removed", C.c_uint32), ("balanced", C.c_uint32),
                ("bad_index", C.c_uint32), ("truncated", C.c_uint32)]


class Peer(C.Structure):
    """udpdk_peer_t: a lane's peer record (raw ip / port), 8 bytes."""
    _fields_ = [("ip", C.c_uint32), ("port", C.c_uint16), ("on", C.c_uint16)]


PEER_DTYPE = np.dtype([("ip", "<u4"), ("port", "<u2"), ("on", "<u2")])   # udpdk_peer_t as a numpy record


class RxPeerStats(C.Structure):
    _fields_ = [("kept", C.c_uint32), ("removed", C.c_uint32), ("refused", C.c_uint32),
                ("bad_frame", C.c_uint32), ("bad_index", C.c_uint32), ("truncated", C.c_uint32)]


MCAST_DTYPE = np.dtype([("group", "<u4"), ("lane", "<u4")])   # udpdk_mcast_member_t as a numpy record
MCAST_MAX_SLOTS = 1 << 20


class RxMcastStats(C.Structure):
    _fields_ = [("kept", C.c_uint32), ("removed", C.c_uint32), ("member", C.c_uint32),
                ("not_member", C.c_uint32), ("bad_frame", C.c_uint32), ("bad_index", C.c_uint32),
                ("truncated", C.c_uint32)]


BAL_TILE = 1024           # frames per rx_balance_pick workgroup (rx_balance.h)
BAL_KEEP_ALL = 0xFFFFFFFF
REUSEPORT_FANOUT, REUSEPORT_BALANCE = 0, 1   # UDPDK_REUSEPORT_*


class RxGather(C.Structure):
    _fields_ = [("payload_dev", C.c_void_p), ("slot_bytes", C.c_uint32), ("len_dev", C.c_void_p),
                ("src_ip_dev", C.c_void_p), ("src_port_dev", C.c_void_p)]


RS_N = 11                 # udpdk_rs_stat
RS_STATS = ("frags", "drop_len", "drop_short", "no_space", "errors", "holes", "expired", "done",
            "stored", "serial", "sorted")


class FragTableCfg(C.Structure):
    _fields_ = [("bucket_num", C.c_uint32), ("bucket_entries", C.c_uint32),
                ("max_cycles", C.c_uint64), ("max_dgram", C.c_uint32), ("max_entries", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


FRAG_CKSUM_DPDK = 1       # UDPDK_FRAG_CKSUM_DPDK
TX_UDP_CKSUM = 1          # UDPDK_TX_UDP_CKSUM


class ReasmOut(C.Structure):
    _fields_ = [("batch", RxBatch), ("origin_dev", C.c_void_p), ("stats", C.c_uint64 * RS_N)]


class RssConf(C.Structure):
    _fields_ = [("key", C.c_uint8 * 40), ("hash_types", C.c_uint32), ("n_queues", C.c_uint32),
                ("reta_size", C.c_uint32), ("reta", C.c_uint16 * 512)]


class RssOut(C.Structure):
    _fields_ = [("hash_dev", C.c_void_p), ("queue_off_dev", C.c_void_p), ("queue_pkt_dev", C.c_void_p)]


class TxConfig(C.Structure):
    _fields_ = [("src_mac", C.c_uint8 * 6), ("dst_mac", C.c_uint8 * 6), ("src_ip", C.c_uint32)]


class TxBatch(C.Structure):
    _fields_ = [("payload_dev", C.c_void_p), ("payload_bytes", C.c_uint64),
                ("payload_off_dev", C.c_void_p), ("payload_len_dev", C.c_void_p),
                ("sockfd_dev", C.c_void_p), ("dst_ip_dev", C.c_void_p),
                ("dst_port_dev", C.c_void_p), ("n", C.c_uint32)]


RX_BURST_FN = C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                          C.c_uint32)
TX_BURST_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32)


class PortOps(C.Structure):
    """udpdk_port_ops_t (udpdk_api.h): a port for the poller thread."""
    _fields_ = [("rx_burst", RX_BURST_FN), ("tx_burst", TX_BURST_FN), ("user", C.c_void_p),
                ("batch_frames", C.c_uint32)]


class TxOut(C.Structure):
    _fields_ = [("frames_dev", C.c_void_p), ("frames_bytes", C.c_uint64),
                ("frame_off_dev", C.c_void_p)]


class TxReplyPlan(C.Structure):
    """udpdk_tx_reply_plan_t: all [count] except frame_off_dev [count + 1]."""
    _fields_ = [("payload_off_dev", C.c_void_p), ("payload_len_dev", C.c_void_p),
                ("sockfd_dev", C.c_void_p), ("dst_ip_dev", C.c_void_p),
                ("dst_port_dev", C.c_void_p), ("frame_off_dev", C.c_void_p)]


class TxReplyStats(C.Structure):
    _fields_ = [("bytes_needed", C.c_uint64), ("replied", C.c_uint32), ("skipped", C.c_uint32),
                ("bad_index", C.c_uint32), ("unselected", C.c_uint32), ("no_room", C.c_uint32),
                ("frames", C.c_uint32)]


GSO_MAX_SEGS = 64         # UDPDK_GSO_MAX_SEGS
SOL_UDP, UDP_SEGMENT = 17, 103


class TxSends(C.Structure):
    """udpdk_tx_sends_t: the arrays are [k]."""
    _fields_ = [("payload_dev", C.c_void_p), ("payload_bytes", C.c_uint64), ("payload_off_dev", C.c_void_p),
                ("payload_len_dev", C.c_void_p), ("gso_size_dev", C.c_void_p), ("sockfd_dev", C.c_void_p),
                ("dst_ip_dev", C.c_void_p), ("dst_port_dev", C.c_void_p), ("k", C.c_uint32)]


class TxSegmentPlan(C.Structure):
    """udpdk_tx_segment_plan_t: all [max_segs] except frame_off_dev [max_segs + 1], seg_off_dev [k + 1]."""
    _fields_ = [("payload_off_dev", C.c_void_p), ("payload_len_dev", C.c_void_p), ("sockfd_dev", C.c_void_p),
                ("dst_ip_dev", C.c_void_p), ("dst_port_dev", C.c_void_p), ("frame_off_dev", C.c_void_p),
                ("seg_off_dev", C.c_void_p), ("max_segs", C.c_uint32)]


SEGMENT_STATS = ("bytes_needed", "segs_needed", "sends", "segments", "frames", "skipped", "too_long", "bad_range",
                 "too_many", "no_room")


class TxSegmentStats(C.Structure):
    """udpdk_tx_segment_stats_t"""
    _fields_ = [(k, C.c_uint64 if k.endswith("_needed") else C.c_uint32) for k in SEGMENT_STATS]


class GsoCounts(C.Structure):
    """udpdk_gso_counts_t (udpdk_api.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("sends", "segments", "plans", "refused")]


class IoVec(C.Structure):
    _fields_ = [("iov_base", C.c_void_p), ("iov_len", C.c_size_t)]


class MsgHdr(C.Structure):
    """struct msghdr (Linux, 64-bit)"""
    _fields_ = [("msg_name", C.c_void_p), ("msg_namelen", C.c_uint32), ("msg_iov", C.POINTER(IoVec)),
                ("msg_iovlen", C.c_size_t), ("msg_control", C.c_void_p), ("msg_controllen", C.c_size_t),
                ("msg_flags", C.c_int)]


ICMP_ECHO, ICMP_UNREACH, ICMP_ALL, ICMP_UNREACH_BYTES = 1, 2, 3, 70


class IcmpOut(C.Structure):
    """udpdk_icmp_out_t"""
    _fields_ = [("frames_dev", C.c_void_p), ("out_cap", C.c_uint64), ("reply_off_dev", C.c_void_p),
                ("origin_dev", C.c_void_p), ("max_replies", C.c_uint32)]


class IcmpStats(C.Structure):
    _fields_ = [("bytes_needed", C.c_uint64), ("replies", C.c_uint32), ("echo_replied", C.c_uint32),
                ("unreach_sent", C.c_uint32), ("echo_bad", C.c_uint32), ("limited", C.c_uint32),
                ("no_room", C.c_uint32), ("bad_frame", C.c_uint32)]


class IcmpCounts(C.Structure):
    """udpdk_icmp_counts_t (udpdk_api.h)"""
    _fields_ = [("echo_replied", C.c_uint64), ("unreach_sent", C.c_uint64), ("echo_bad", C.c_uint64),
                ("limited", C.c_uint64), ("queue_dropped", C.c_uint64)]


class ArpOut(C.Structure):
    """udpdk_arp_out_t"""
    _fields_ = [("frames_dev", C.c_void_p), ("origin_dev", C.c_void_p), ("max_replies", C.c_uint32)]


ARP_STATS = ("arp", "malformed", "other_op", "own", "sender_bad", "not_ours", "conflict", "eligible", "replies",
             "no_room", "bad_frame")
ARP_FRAME_BYTES = 42
ARP_SLOT_BYTES = 64


class ArpStats(C.Structure):
    """udpdk_arp_stats_t"""
    _fields_ = [(k, C.c_uint32) for k in ARP_STATS]


class IgmpOut(C.Structure):
    """udpdk_igmp_out_t"""
    _fields_ = [("frames_dev", C.c_void_p), ("group_index_dev", C.c_void_p), ("max_reports", C.c_uint32)]


IGMP_STATS = ("igmp", "malformed", "bad_cksum", "other_type", "bad_dst", "general", "not_member", "specific",
              "reports", "no_room", "bad_frame")
IGMP_FRAME_BYTES = 46
IGMP_SLOT_BYTES = 64
IGMP_MAX_GROUPS = 4096


class IgmpStats(C.Structure):
    """udpdk_igmp_stats_t"""
    _fields_ = [(k, C.c_uint32) for k in IGMP_STATS]


class McastCounts(C.Structure):
    """udpdk_mcast_counts_t (udpdk_api.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("scanned", "igmp", "malformed", "bad_cksum", "other_type", "bad_dst", "general",
                                          "not_member", "specific", "reports", "joins", "leaves", "reports_sent",
                                          "leaves_sent")]


IPPROTO_IP, IP_ADD_MEMBERSHIP, IP_DROP_MEMBERSHIP = 0, 35, 36


class ArpCounts(C.Structure):
    """udpdk_arp_counts_t (udpdk_api.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("scanned",) + ARP_STATS[:-1] + ("announced",)]


NEIGH_EMPTY, NEIGH_INCOMPLETE, NEIGH_REACHABLE, NEIGH_STATIC = range(4)
NEIGH_FALLBACK = 1
NEIGH_MAX_ENTRIES = 65536
(NEIGH_C_SKIPPED, NEIGH_C_BCAST, NEIGH_C_MCAST, NEIGH_C_NO_ROUTE, NEIGH_C_SELF, NEIGH_C_HIT, NEIGH_C_EXPIRED,
 NEIGH_C_INCOMPLETE, NEIGH_C_INSERTED, NEIGH_C_TABLE_FULL) = range(10)
NEIGH_C_LOOKUP = NEIGH_C_HIT
NEIGH_HASH_K = 0x9E3779B1
NEIGH_LEARN_STATS = ("arp", "malformed", "bad_frame", "other_op", "sender_bad", "updated", "refreshed", "static_kept",
                     "created", "full", "ignored")
NEIGH_RESOLVE_STATS = ("skipped", "bcast", "mcast", "no_route", "self", "hit", "expired", "incomplete", "inserted",
                       "table_full", "fallback", "unresolved", "requests", "no_room")


class NeighEntry(C.Structure):
    """udpdk_neigh_entry_t"""
    _fields_ = [("ip", C.c_uint32), ("mac", C.c_uint8 * 6), ("state", C.c_uint8), ("pad", C.c_uint8),
                ("stamp", C.c_uint32)]


class NeighCfg(C.Structure):
    """udpdk_neigh_cfg_t"""
    _fields_ = [("src_ip", C.c_uint32), ("netmask", C.c_uint32), ("gateway", C.c_uint32), ("src_mac", C.c_uint8 * 6),
                ("fallback_mac", C.c_uint8 * 6), ("ttl_ms", C.c_uint32), ("retrans_ms", C.c_uint32),
                ("flags", C.c_uint32)]


class NeighLearnStats(C.Structure):
    """udpdk_neigh_learn_stats_t"""
    _fields_ = [(k, C.c_uint32) for k in NEIGH_LEARN_STATS]


class NeighOut(C.Structure):
    """udpdk_neigh_out_t"""
    _fields_ = [("dmac_dev", C.c_void_p), ("sockfd_out_dev", C.c_void_p), ("state_dev", C.c_void_p),
                ("req_dev", C.c_void_p), ("req_origin_dev", C.c_void_p), ("req_cap", C.c_uint32)]


class NeighResolveStats(C.Structure):
    """udpdk_neigh_resolve_stats_t"""
    _fields_ = [(k, C.c_uint32) for k in NEIGH_RESOLVE_STATS]


class NeighCounts(C.Structure):
    """udpdk_neigh_counts_t (udpdk_api.h)"""
    _fields_ = [(k, C.c_uint64) for k in NEIGH_LEARN_STATS + NEIGH_RESOLVE_STATS[:-2] + ("no_room", "tx_unresolved",
                                                                                        "requests")]


class IcmpErrStats(C.Structure):
    """udpdk_icmp_err_stats_t"""
    _fields_ = [("errors", C.c_uint32), ("msg_bad", C.c_uint32), ("quote_bad", C.c_uint32), ("soft", C.c_uint32),
                ("no_socket", C.c_uint32), ("reported", C.c_uint32), ("bad_frame", C.c_uint32)]


class IcmpErrCounts(C.Structure):
    """udpdk_icmp_err_counts_t (udpdk_api.h)"""
    _fields_ = [("errors", C.c_uint64), ("msg_bad", C.c_uint64), ("quote_bad", C.c_uint64), ("soft", C.c_uint64),
                ("no_socket", C.c_uint64), ("reported", C.c_uint64), ("posted", C.c_uint64)]


ICMP_ERR_STATS = ("errors", "msg_bad", "quote_bad", "soft", "no_socket", "reported", "bad_frame")

# name -> (restype, argtypes); every symbol the headers declare
_P = C.c_void_p
_PROTOS = {
    # udpdk_gpu.h
    "udpdk_gpu_abi_version": (C.c_int, []),
    "udpdk_gpu_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "udpdk_gpu_ctx_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "udpdk_gpu_ctx_destroy": (C.c_int, [_P]),
    "udpdk_gpu_sync": (C.c_int, [_P]),
    "udpdk_gpu_last_hip_error": (C.c_int, [_P]),
    "udpdk_gpu_stream": (_P, [_P]),
    "udpdk_gpu_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "udpdk_gpu_free": (C.c_int, [_P, _P]),
    "udpdk_gpu_host_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "udpdk_gpu_host_free": (C.c_int, [_P, _P]),
    "udpdk_gpu_memset": (C.c_int, [_P, _P, C.c_int, C.c_size_t]),
    "udpdk_gpu_h2d": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "udpdk_gpu_d2h": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "udpdk_gpu_bind_snapshot_upload": (C.c_int, [_P, C.POINTER(BindSnapshot)]),
    "udpdk_gpu_rx": (C.c_int, [_P, C.POINTER(RxBatch), C.POINTER(RxOut)]),
    "udpdk_gpu_rx_stats": (C.c_int, [_P, C.POINTER(RxStats)]),
    "udpdk_gpu_pipeline_depth": (C.c_int, [_P, C.c_int]),
    "udpdk_gpu_join": (C.c_int, [_P]),
    "udpdk_gpu_rx_host": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, C.c_uint32, _P, _P, _P,
                                    C.c_uint32, C.POINTER(RxStats)]),
    "udpdk_gpu_rx_host_async": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, C.c_uint32, _P, _P, _P,
                                          C.c_uint32, C.POINTER(RxStats)]),
    "udpdk_gpu_rx_host_wait": (C.c_int, [_P]),
    "udpdk_gpu_rx_host_batch": (C.c_int, [_P, C.POINTER(RxBatch), C.POINTER(_P)]),
    # poller internals (udpdk_poll_rx's pipelined form)
    "udpdk_gpu_pipe_rx_host": (C.c_int, [_P, C.c_int, _P, C.c_uint64, _P, C.c_uint32, _P, _P, C.c_uint32,
                                         _P, _P, _P, C.c_uint32, C.POINTER(RxStats)]),
    "udpdk_gpu_pipe_wait": (C.c_int, [_P, C.c_int]),
    "udpdk_gpu_pipe_batch": (C.c_int, [_P, C.c_int, C.POINTER(RxBatch), C.POINTER(_P)]),
    "udpdk_gpu_pipe_h2d": (C.c_int, [_P, C.c_int, _P, _P, C.c_size_t]),
    "udpdk_gpu_pipe_d2h": (C.c_int, [_P, C.c_int, _P, _P, C.c_size_t]),
    "udpdk_gpu_pipe_gather_packed": (C.c_int, [_P, C.c_int, C.POINTER(RxBatch), _P, C.c_uint32, C.c_uint32,
                                               _P, C.POINTER(RxGather)]),
    "udpdk_gpu_rx_filter": (C.c_int, [_P, C.POINTER(RxLanes), C.c_uint32, _P, _P, C.c_uint32]),
    "udpdk_gpu_rx_drop": (C.c_int, [_P, C.c_int]),
    "udpdk_gpu_rx_drop_stats": (C.c_int, [_P, C.POINTER(RxDropStats)]),
    "udpdk_gpu_rx_balance_select": (C.c_int, [_P, C.POINTER(RxBatch), C.POINTER(RxLanes), _P, _P, _P, _P,
                                              C.c_uint32]),
    "udpdk_gpu_rx_balance": (C.c_int, [_P, _P, C.c_uint32]),
    "udpdk_gpu_rx_balance_stats": (C.c_int, [_P, C.POINTER(RxBalanceStats)]),
    "udpdk_gpu_rx_balance_rank": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "udpdk_gpu_rx_removed": (C.c_int, [_P, C.POINTER(RxStats), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "udpdk_gpu_rx_peer_select": (C.c_int, [_P, C.POINTER(RxBatch), C.POINTER(RxLanes), _P, _P, _P, C.c_uint32]),
    "udpdk_gpu_rx_peer": (C.c_int, [_P, _P, C.c_uint32]),
    "udpdk_gpu_rx_peer_stats": (C.c_int, [_P, C.POINTER(RxPeerStats)]),
    "udpdk_gpu_rx_peer_removed": (C.c_int, [_P, C.POINTER(RxStats), C.POINTER(C.c_uint32)]),
    "udpdk_gpu_mcast_table_build": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32]),
    "udpdk_gpu_rx_mcast_select": (C.c_int, [_P, C.POINTER(RxBatch), C.POINTER(RxLanes), _P, _P, C.c_uint32, _P, _P,
                                            C.c_uint32]),
    "udpdk_gpu_rx_mcast": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32]),
    "udpdk_gpu_rx_mcast_stats": (C.c_int, [_P, C.POINTER(RxMcastStats)]),
    "udpdk_gpu_rx_mcast_removed": (C.c_int, [_P, C.POINTER(RxStats), C.POINTER(C.c_uint32)]),
    "udpdk_gpu_rx_gather": (C.c_int, [_P, C.POINTER(RxBatch), _P, C.c_uint32, C.c_uint32,
                                      C.POINTER(RxGather)]),
    "udpdk_gpu_rx_gather_packed": (C.c_int, [_P, C.POINTER(RxBatch), _P, C.c_uint32, C.c_uint32, _P,
                                             C.POINTER(RxGather)]),
    "udpdk_gpu_frag_table_create": (C.c_int, [_P, C.POINTER(FragTableCfg)]),
    "udpdk_gpu_rx_reassemble": (C.c_int, [_P, C.POINTER(RxBatch), _P, C.c_uint64, C.POINTER(ReasmOut)]),
    "udpdk_gpu_rx_reassemble_inplace": (C.c_int, [_P, C.POINTER(RxBatch), _P, C.c_uint64, C.POINTER(ReasmOut)]),
    "udpdk_gpu_rss_default_conf": (C.c_int, [C.POINTER(RssConf), C.c_uint32]),
    "udpdk_gpu_rss_config": (C.c_int, [_P, C.POINTER(RssConf)]),
    "udpdk_gpu_rss": (C.c_int, [_P, C.POINTER(RxBatch), C.POINTER(RssOut)]),
    "udpdk_gpu_tx_build": (C.c_int, [_P, C.POINTER(TxConfig), C.POINTER(TxBatch), C.POINTER(TxOut)]),
    "udpdk_gpu_tx_build_mtu": (C.c_int, [_P, C.POINTER(TxConfig), C.POINTER(TxBatch),
                                         C.POINTER(TxOut), C.c_uint32]),
    "udpdk_gpu_tx_build_flags": (C.c_int, [_P, C.POINTER(TxConfig), C.POINTER(TxBatch),
                                           C.POINTER(TxOut), C.c_uint32, C.c_uint32]),
    "udpdk_gpu_tx_span": (C.c_uint64, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "udpdk_gpu_tx_reply_plan": (C.c_int, [_P, C.POINTER(RxBatch), C.POINTER(RxLanes), C.c_uint32, C.c_uint32,
                                          _P, C.c_uint32, C.c_uint64, C.POINTER(TxReplyPlan)]),
    "udpdk_gpu_tx_reply": (C.c_int, [_P, C.POINTER(TxConfig), C.POINTER(RxBatch), C.POINTER(RxLanes),
                                     C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, C.c_uint64,
                                     C.POINTER(TxReplyPlan)]),
    "udpdk_gpu_tx_reply_stats": (C.c_int, [_P, C.POINTER(TxReplyStats)]),
    "udpdk_gpu_tx_reply_geometry": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "udpdk_gpu_tx_segment_plan": (C.c_int, [_P, C.POINTER(TxSends), C.c_uint32, C.c_uint32, C.c_uint64,
                                            C.POINTER(TxSegmentPlan)]),
    "udpdk_gpu_tx_segment": (C.c_int, [_P, C.POINTER(TxConfig), C.POINTER(TxSends), C.c_uint32, C.c_uint32, C.c_uint32,
                                       _P, C.c_uint64, C.POINTER(TxSegmentPlan)]),
    "udpdk_gpu_tx_segment_stats": (C.c_int, [_P, C.POINTER(TxSegmentStats)]),
    "udpdk_gpu_tx_segment_span": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                               C.POINTER(C.c_uint32)]),
    "udpdk_gpu_tx_segment_geometry": (C.c_int, [C.c_uint32, C.c_uint32] + [C.POINTER(C.c_uint32)] * 4),
    "udpdk_gpu_icmp_reply": (C.c_int, [_P, C.POINTER(TxConfig), C.POINTER(RxBatch), _P, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.POINTER(IcmpOut)]),
    "udpdk_gpu_icmp_stats": (C.c_int, [_P, C.POINTER(IcmpStats)]),
    "udpdk_gpu_icmp_geometry": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "udpdk_gpu_pipe_icmp_reply": (C.c_int, [_P, C.c_int, C.POINTER(TxConfig), C.POINTER(RxBatch), _P, C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.POINTER(IcmpOut)]),
    "udpdk_gpu_pipe_icmp_stats": (C.c_int, [_P, C.c_int, C.POINTER(IcmpStats)]),
    "udpdk_gpu_icmp_errors": (C.c_int, [_P, C.c_uint32, C.POINTER(RxBatch), _P, _P, C.c_uint32, _P]),
    "udpdk_gpu_icmp_err_stats": (C.c_int, [_P, C.POINTER(IcmpErrStats)]),
    "udpdk_gpu_pipe_icmp_errors": (C.c_int, [_P, C.c_int, C.c_uint32, C.POINTER(RxBatch), _P, _P, C.c_uint32, _P]),
    "udpdk_gpu_pipe_icmp_err_stats": (C.c_int, [_P, C.c_int, C.POINTER(IcmpErrStats)]),
    "udpdk_gpu_icmp_errno": (C.c_int, [C.c_uint32, C.POINTER(C.c_int)]),
    "udpdk_gpu_arp_reply": (C.c_int, [_P, C.POINTER(TxConfig), C.POINTER(RxBatch), _P, C.POINTER(ArpOut)]),
    "udpdk_gpu_arp_stats": (C.c_int, [_P, C.POINTER(ArpStats)]),
    "udpdk_gpu_arp_geometry": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "udpdk_gpu_pipe_arp_reply": (C.c_int, [_P, C.c_int, C.POINTER(TxConfig), C.POINTER(RxBatch), _P,
                                           C.POINTER(ArpOut)]),
    "udpdk_gpu_pipe_arp_stats": (C.c_int, [_P, C.c_int, C.POINTER(ArpStats)]),
    "udpdk_gpu_igmp_reply": (C.c_int, [_P, C.POINTER(TxConfig), C.POINTER(RxBatch), _P, _P, C.c_uint32,
                                       C.POINTER(IgmpOut)]),
    "udpdk_gpu_igmp_stats": (C.c_int, [_P, C.POINTER(IgmpStats)]),
    "udpdk_gpu_igmp_geometry": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "udpdk_gpu_pipe_igmp_reply": (C.c_int, [_P, C.c_int, C.POINTER(TxConfig), C.POINTER(RxBatch), _P, _P, C.c_uint32,
                                            C.POINTER(IgmpOut)]),
    "udpdk_gpu_pipe_igmp_stats": (C.c_int, [_P, C.c_int, C.POINTER(IgmpStats)]),
    "udpdk_gpu_neigh_create": (C.c_int, [_P, C.c_uint32]),
    "udpdk_gpu_neigh_set": (C.c_int, [_P, C.POINTER(NeighEntry), C.c_uint32]),
    "udpdk_gpu_neigh_dump": (C.c_int, [_P, C.POINTER(NeighEntry), C.c_uint32, C.POINTER(C.c_uint32)]),
    "udpdk_gpu_neigh_flush": (C.c_int, [_P, C.c_int]),
    "udpdk_gpu_neigh_learn": (C.c_int, [_P, C.POINTER(NeighCfg), C.POINTER(RxBatch), _P, C.c_uint32]),
    "udpdk_gpu_neigh_learn_stats": (C.c_int, [_P, C.POINTER(NeighLearnStats)]),
    "udpdk_gpu_pipe_neigh_learn": (C.c_int, [_P, C.c_int, C.POINTER(NeighCfg), C.POINTER(RxBatch), _P, C.c_uint32]),
    "udpdk_gpu_pipe_neigh_learn_stats": (C.c_int, [_P, C.c_int, C.POINTER(NeighLearnStats)]),
    "udpdk_gpu_neigh_resolve": (C.c_int, [_P, C.POINTER(NeighCfg), _P, _P, C.c_uint32, C.c_uint32,
                                          C.POINTER(NeighOut)]),
    "udpdk_gpu_neigh_resolve_stats": (C.c_int, [_P, C.POINTER(NeighResolveStats)]),
    "udpdk_gpu_neigh_geometry": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "udpdk_gpu_neigh_class": (C.c_int, [C.POINTER(NeighCfg), C.c_uint32, C.POINTER(C.c_uint32), _P]),
    "udpdk_gpu_tx_build_neigh": (C.c_int, [_P, C.POINTER(TxConfig), C.POINTER(TxBatch), C.POINTER(TxOut), C.c_uint32,
                                           C.c_uint32, _P]),
    "udpdk_gpu_timing_enable": (C.c_int, [_P, C.c_int]),
    "udpdk_gpu_timing_read": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    "udpdk_gpu_rx_geometry": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32)]),
    # udpdk_api.h
    "udpdk_init": (C.c_int, [C.c_int, C.POINTER(C.c_char_p)]),
    "udpdk_interrupt": (None, [C.c_int]),
    "udpdk_cleanup": (None, []),
    "udpdk_socket": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "udpdk_getsockopt": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_uint32)]),
    "udpdk_setsockopt": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_uint32]),
    "udpdk_bind": (C.c_int, [C.c_int, _P, C.c_uint32]),
    "udpdk_sendto": (C.c_ssize_t, [C.c_int, _P, C.c_size_t, C.c_int, _P, C.c_uint32]),
    "udpdk_recvfrom": (C.c_ssize_t, [C.c_int, _P, C.c_size_t, C.c_int, _P, C.POINTER(C.c_uint32)]),
    "udpdk_close": (C.c_int, [C.c_int]),
    "udpdk_connect": (C.c_int, [C.c_int, _P, C.c_uint32]),
    "udpdk_send": (C.c_ssize_t, [C.c_int, _P, C.c_size_t, C.c_int]),
    "udpdk_recv": (C.c_ssize_t, [C.c_int, _P, C.c_size_t, C.c_int]),
    "udpdk_getpeername": (C.c_int, [C.c_int, _P, C.POINTER(C.c_uint32)]),
    "udpdk_getsockname": (C.c_int, [C.c_int, _P, C.POINTER(C.c_uint32)]),
    "udpdk_rx_refused": (C.c_uint64, []),
    "udpdk_peer_lanes": (C.c_int, [_P, C.c_uint32]),
    "udpdk_dump_payload": (None, [C.c_char_p, C.c_int]),
    "udpdk_poll_rx": (C.c_int, [_P, C.c_uint64, _P, _P, _P, C.c_uint32, C.POINTER(RxStats)]),
    "udpdk_tx_drain": (C.c_int, [_P, C.c_uint64, _P, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    "udpdk_poll_echo": (C.c_int, [_P, C.c_uint64, _P, _P, _P, C.c_uint32, _P, C.c_uint64, _P, _P, C.c_uint32,
                                  C.POINTER(C.c_uint32), C.POINTER(RxStats)]),
    "udpdk_btable_snapshot": (C.c_int, [C.POINTER(BindSnapshot), C.c_int]),
    "udpdk_gpu_context": (_P, []),
    "udpdk_shard_devices": (C.c_int, [_P, C.c_int]),
    "udpdk_shard_plan": (C.c_int, [C.c_char_p, _P, C.c_int]),
    "udpdk_shard_frames": (C.c_int, [_P, C.c_int]),
    "udpdk_config_set": (C.c_int, [_P, _P, C.c_uint32]),
    "udpdk_config_get": (C.c_int, [_P, _P, C.POINTER(C.c_uint32)]),
    "udpdk_config_mtu": (C.c_int, [C.c_uint32]),
    "udpdk_config_tx_cksum": (C.c_int, [C.c_int]),
    "udpdk_config_rx_drop": (C.c_int, [C.c_int]),
    "udpdk_rx_dropped": (C.c_uint64, []),
    "udpdk_config_reuseport": (C.c_int, [C.c_int]),
    "udpdk_rx_balanced": (C.c_uint64, []),
    "udpdk_reuseport_lanes": (C.c_int, [_P, C.c_uint32]),
    "udpdk_config_icmp": (C.c_int, [C.c_int]),
    "udpdk_config_icmp_burst": (C.c_int, [C.c_int]),
    "udpdk_icmp_counts": (C.c_int, [C.POINTER(IcmpCounts)]),
    "udpdk_config_icmp_errors": (C.c_int, [C.c_int]),
    "udpdk_config_arp": (C.c_int, [C.c_int]),
    "udpdk_arp_announce": (C.c_int, []),
    "udpdk_config_mcast": (C.c_int, [C.c_int]),
    "udpdk_mcast_counts": (C.c_int, [C.POINTER(McastCounts)]),
    "udpdk_rx_not_member": (C.c_uint64, []),
    "udpdk_arp_counts": (C.c_int, [C.POINTER(ArpCounts)]),
    "udpdk_config_neigh": (C.c_int, [C.c_int]),
    "udpdk_neigh_add": (C.c_int, [C.c_uint32, _P]),
    "udpdk_neigh_flush": (C.c_int, []),
    "udpdk_neigh_counts": (C.c_int, [C.POINTER(NeighCounts)]),
    "udpdk_sendmsg": (C.c_ssize_t, [C.c_int, C.POINTER(MsgHdr), C.c_int]),
    "udpdk_gso_counts": (C.c_int, [C.POINTER(GsoCounts)]),
    "udpdk_sock_error_post": (C.c_int, [C.c_int, C.c_uint32, C.c_uint16, C.c_uint32]),
    "udpdk_icmp_err_counts": (C.c_int, [C.POINTER(IcmpErrCounts)]),
    "udpdk_sock_rx_inject": (C.c_int, [C.c_int, _P, C.c_uint32, C.c_uint32, C.c_uint16]),
    "udpdk_tx_pending": (C.c_uint64, []),
    "udpdk_tx_dropped": (C.c_uint64, []),
    "udpdk_rx_nobufs": (C.c_uint64, []),
    "udpdk_port_attach": (C.c_int, [C.POINTER(PortOps)]),
    "udpdk_port_detach": (C.c_int, []),
    "udpdk_port_loopback": (C.c_int, [C.POINTER(PortOps)]),
    "udpdk_slot_table": (C.c_int, [C.POINTER(Slot), C.c_uint32]),
    "udpdk_host_reset": (None, []),
}

_lib = None


def lib() -> C.CDLL:
    """Load libudpdk_amd.so (raises if it was not built: there is no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run `make` (or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _PROTOS.items():
            try:
                f = getattr(L, name)
            except AttributeError:
                # an A/B build of an older tree (tools/ab.py) may predate a newer entry point
                if os.environ.get("UDPDK_LIB_OVERRIDE"):
                    continue
                raise
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def declared_symbols() -> list[str]:
    return sorted(_PROTOS)


class UdpdkError(RuntimeError):
    pass


def _check(rc: int, what: str):
    if rc != 0:
        raise UdpdkError(f"{what} failed: rc={rc} ({errno.errorcode.get(-rc, '?')})")


def device_count() -> int:
    n = C.c_int(0)
    lib().udpdk_gpu_device_count(C.byref(n))
    return n.value


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


# ---- snapshot construction from Python binding lists -------------------------------------------
@dataclass
class HostSnapshot:
    """Arrays behind a BindSnapshot (kept alive with the struct)."""
    port_first: np.ndarray
    port_count: np.ndarray
    binds: C.Array
    slots: C.Array | None
    snap: BindSnapshot


def snapshot_from_lists(port_lists: dict[int, list[tuple[int, int, int]]], n_lanes: int,
                        lane_mask: int = 0xFFFFFFFF, slots: list[tuple[int, int, int]] | None = None
                        ) -> HostSnapshot:
    """port_lists: raw port -> [(ip_raw, sockfd, reuse)] in list (head -> tail) order."""
    first = np.zeros(65536, np.uint32)
    count = np.zeros(65536, np.uint16)
    flat = []
    for p in sorted(port_lists):
        lst = port_lists[p]
        if not lst:
            continue
        first[p] = len(flat)
        count[p] = len(lst)
        flat.extend(lst)
    arr = (Binding * max(1, len(flat)))()
    for i, (ip, sock, reuse) in enumerate(flat):
        arr[i].ip, arr[i].sockfd, arr[i].reuse = ip, sock, reuse
    sl = None
    if slots:
        sl = (Slot * len(slots))()
        for i, (ip, port, bound) in enumerate(slots):
            sl[i].ip, sl[i].udp_port, sl[i].bound = ip, port, bound
    snap = BindSnapshot(first.ctypes.data_as(C.POINTER(C.c_uint32)),
                        count.ctypes.data_as(C.POINTER(C.c_uint16)),
                        C.cast(arr, C.POINTER(Binding)), len(flat), n_lanes, lane_mask,
                        C.cast(sl, C.POINTER(Slot)) if sl is not None else None,
                        len(slots) if slots else 0, 1)
    return HostSnapshot(first, count, arr, sl, snap)


# ---- device context ------------------------------------------------------------------------------
class DeviceBuffer:
    def __init__(self, ctx: "GpuContext", nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _check(lib().udpdk_gpu_alloc(ctx.handle, max(1, self.nbytes), C.byref(p)), "udpdk_gpu_alloc")
        self.ptr = p.value

    def free(self):
        if self.ptr:
            lib().udpdk_gpu_free(self.ctx.handle, C.c_void_p(self.ptr))
            self.ptr = None


class GpuContext:
    """A udpdk_gpu_ctx on one device."""

    def __init__(self, device: int = 0, max_frames: int = 1 << 20, max_lanes: int = 4096):
        h = C.c_void_p()
        _check(lib().udpdk_gpu_ctx_create(device, max_frames, max_lanes, C.byref(h)),
               "udpdk_gpu_ctx_create")
        self.handle = h
        self.device = device
        self._bufs: list[DeviceBuffer] = []

    def close(self):
        for b in self._bufs:
            b.free()
        self._bufs.clear()
        if self.handle:
            lib().udpdk_gpu_ctx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def alloc(self, nbytes: int) -> DeviceBuffer:
        b = DeviceBuffer(self, nbytes)
        self._bufs.append(b)
        return b

    def upload(self, a: np.ndarray) -> DeviceBuffer:
        a = np.ascontiguousarray(a)
        b = self.alloc(a.nbytes)
        if a.nbytes:
            _check(lib().udpdk_gpu_h2d(self.handle, C.c_void_p(b.ptr), C.c_void_p(_ptr(a)), a.nbytes), "h2d")
            self.sync()
        return b

    def download(self, b: DeviceBuffer, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype)
        if out.nbytes:
            _check(lib().udpdk_gpu_d2h(self.handle, C.c_void_p(_ptr(out)), C.c_void_p(b.ptr), out.nbytes), "d2h")
            self.sync()
        return out

    def sync(self):
        _check(lib().udpdk_gpu_sync(self.handle), "udpdk_gpu_sync")

    def pipeline(self, depth: int):
        """1: every udpdk_gpu_rx in order on one stream; 2: consecutive calls alternate between
        two streams (independent batches with distinct outputs overlap)."""
        _check(lib().udpdk_gpu_pipeline_depth(self.handle, int(depth)), "udpdk_gpu_pipeline_depth")

    def join(self):
        _check(lib().udpdk_gpu_join(self.handle), "udpdk_gpu_join")

    def upload_snapshot(self, hs: HostSnapshot):
        _check(lib().udpdk_gpu_bind_snapshot_upload(self.handle, C.byref(hs.snap)),
               "udpdk_gpu_bind_snapshot_upload")

    def rx_drop(self, flags: int) -> int:
        """Sticky RX drop filter (udpdk_gpu_rx_drop): RX_DROP_* flags for every later RX call on
        the context; returns the previous flags, a negative argument only reads them."""
        rc = lib().udpdk_gpu_rx_drop(self.handle, int(flags))
        if rc < 0:
            _check(rc, "udpdk_gpu_rx_drop")
        return rc

    def rx_balance(self, lane_rp=None):
        """Sticky reuse-port balance (udpdk_gpu_rx_balance): the lanes' SO_REUSEPORT flags for
        every later RX call on the context; None turns the stage off."""
        if lane_rp is None or len(lane_rp) == 0:
            _check(lib().udpdk_gpu_rx_balance(self.handle, None, 0), "udpdk_gpu_rx_balance")
            return
        f = np.ascontiguousarray(lane_rp, np.uint8)
        _check(lib().udpdk_gpu_rx_balance(self.handle, f.ctypes.data_as(C.c_void_p), len(f)),
               "udpdk_gpu_rx_balance")

    def rx_peer(self, peers=None):
        """Sticky peer filter (udpdk_gpu_rx_peer): the lanes' peer records (PEER_DTYPE) for every
        later RX call on the context; None turns the stage off."""
        if peers is None or len(peers) == 0:
            _check(lib().udpdk_gpu_rx_peer(self.handle, None, 0), "udpdk_gpu_rx_peer")
            return
        t = np.ascontiguousarray(peers, PEER_DTYPE)
        _check(lib().udpdk_gpu_rx_peer(self.handle, t.ctypes.data_as(C.c_void_p), len(t)), "udpdk_gpu_rx_peer")

    def rx_mcast(self, lane_mc=None, members=None):
        """Sticky membership filter (udpdk_gpu_rx_mcast): the lanes' checked flags and the (group,
        lane) members (MCAST_DTYPE) for every later RX call on the context; lane_mc None turns the
        stage off."""
        if lane_mc is None or len(lane_mc) == 0:
            _check(lib().udpdk_gpu_rx_mcast(self.handle, None, 0, None, 0), "udpdk_gpu_rx_mcast")
            return
        f = np.ascontiguousarray(lane_mc, np.uint8)
        m = np.ascontiguousarray(members if members is not None else [], MCAST_DTYPE)
        _check(lib().udpdk_gpu_rx_mcast(self.handle, f.ctypes.data_as(C.c_void_p), len(f),
                                        m.ctypes.data_as(C.c_void_p) if len(m) else None, len(m)),
               "udpdk_gpu_rx_mcast")

    def timing(self, every: int):
        """0 = off, N = record kernel events on every Nth udpdk_gpu_rx call."""
        _check(lib().udpdk_gpu_timing_enable(self.handle, int(every)), "timing_enable")

    def timing_read(self):
        ms = (C.c_double * N_KERNEL_IDS)()
        n = (C.c_uint32 * N_KERNEL_IDS)()
        _check(lib().udpdk_gpu_timing_read(self.handle, ms, n), "timing_read")
        return list(ms), list(n)


@dataclass
class RxDeviceBatch:
    frames: DeviceBuffer
    frames_bytes: int
    offset: DeviceBuffer
    length: DeviceBuffer
    ptype: DeviceBuffer | None
    n: int


@dataclass
class RxDeviceOut:
    meta: DeviceBuffer
    lane_off: DeviceBuffer
    lane_pkt: DeviceBuffer
    lane_cap: int
    n: int
    n_lanes: int


FRAMES_TAILROOM = 16    # UDPDK_GPU_FRAMES_TAILROOM


def rx_upload(ctx: GpuContext, frames: np.ndarray, offset: np.ndarray, length: np.ndarray,
              ptype: np.ndarray | None = None) -> RxDeviceBatch:
    """Device copies of a batch; the frames buffer gets UDPDK_GPU_FRAMES_TAILROOM readable bytes
    past the frame data."""
    fb = ctx.alloc(int(frames.nbytes) + FRAMES_TAILROOM)
    _check(lib().udpdk_gpu_h2d(ctx.handle, C.c_void_p(fb.ptr), frames.ctypes.data_as(C.c_void_p),
                               int(frames.nbytes)), "udpdk_gpu_h2d")
    ctx.sync()
    return RxDeviceBatch(fb, int(frames.nbytes), ctx.upload(offset.astype(np.uint32)),
                         ctx.upload(length.astype(np.uint16)),
                         ctx.upload(ptype.astype(np.uint32)) if ptype is not None else None,
                         int(len(offset)))


def rx_alloc_out(ctx: GpuContext, n: int, n_lanes: int, lane_cap: int) -> RxDeviceOut:
    return RxDeviceOut(ctx.alloc(4 * max(1, n)), ctx.alloc(4 * (n_lanes + 1)),
                       ctx.alloc(4 * max(1, lane_cap)), lane_cap, n, n_lanes)


def rx_enqueue(ctx: GpuContext, b: RxDeviceBatch, o: RxDeviceOut) -> int:
    bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                 b.ptype.ptr if b.ptype is not None else None, b.n)
    ot = RxOut(o.meta.ptr, o.lane_off.ptr, o.lane_pkt.ptr, o.lane_cap)
    return lib().udpdk_gpu_rx(ctx.handle, C.byref(bt), C.byref(ot))


def rx_stats(ctx: GpuContext) -> tuple[int, RxStats]:
    st = RxStats()
    rc = lib().udpdk_gpu_rx_stats(ctx.handle, C.byref(st))
    return rc, st


def rx_run(ctx: GpuContext, b: RxDeviceBatch, o: RxDeviceOut):
    """Run the RX pipeline and download (meta, lane_off, lane_pkt[:D], counters)."""
    _check(rx_enqueue(ctx, b, o), "udpdk_gpu_rx")
    rc, st = rx_stats(ctx)
    if rc not in (0, -errno.ENOSPC):
        _check(rc, "udpdk_gpu_rx_stats")
    meta = ctx.download(o.meta, np.uint32, o.n)
    loff = ctx.download(o.lane_off, np.uint32, o.n_lanes + 1)
    d = min(int(st.deliveries), o.lane_cap)
    pkt = ctx.download(o.lane_pkt, np.uint32, d)
    return meta, loff, pkt, np.array(st.counters[:], np.uint64), rc


def rx_drop_stats(ctx: GpuContext) -> tuple[int, RxDropStats]:
    st = RxDropStats()
    rc = lib().udpdk_gpu_rx_drop_stats(ctx.handle, C.byref(st))
    return rc, st


def rx_filter_run(ctx: GpuContext, meta: np.ndarray, lane_off: np.ndarray, lane_pkt: np.ndarray,
                  flags: int, *, n: int | None = None, lane_cap: int | None = None,
                  out_cap: int | None = None, pad: int = 0, fill: int = 0xA5A5A5A5):
    """udpdk_gpu_rx_filter over host arrays: upload, run, download. lane_pkt is uploaded whole
    (lane_cap defaults to its length, so a caller may pass more than lane_off[-1] entries); the
    entry output buffer has out_cap + pad words, all pre-filled with `fill`. Returns (lane_off_out,
    lane_pkt_out[out_cap + pad], RxDropStats, rc of udpdk_gpu_rx_drop_stats)."""
    meta = np.ascontiguousarray(meta, np.uint32)
    lane_off = np.ascontiguousarray(lane_off, np.uint32)
    lane_pkt = np.ascontiguousarray(lane_pkt, np.uint32)
    n = len(meta) if n is None else n
    lane_cap = len(lane_pkt) if lane_cap is None else lane_cap
    out_cap = lane_cap if out_cap is None else out_cap
    n_lanes = len(lane_off) - 1
    bufs = [ctx.upload(meta), ctx.upload(lane_off), ctx.upload(lane_pkt),
            ctx.upload(np.full(n_lanes + 1, fill, np.uint32)),
            ctx.upload(np.full(out_cap + pad, fill, np.uint32))]
    md, od, pd, oo, po = bufs
    try:
        lanes = RxLanes(md.ptr, n, od.ptr, pd.ptr, lane_cap, n_lanes)
        _check(lib().udpdk_gpu_rx_filter(ctx.handle, C.byref(lanes), flags, C.c_void_p(oo.ptr),
                                         C.c_void_p(po.ptr), out_cap), "udpdk_gpu_rx_filter")
        rc, st = rx_drop_stats(ctx)
        return (ctx.download(oo, np.uint32, n_lanes + 1), ctx.download(po, np.uint32, out_cap + pad),
                st, rc)
    finally:
        for b in bufs:
            b.free()


def rx_balance_stats(ctx: GpuContext) -> tuple[int, RxBalanceStats]:
    st = RxBalanceStats()
    rc = lib().udpdk_gpu_rx_balance_stats(ctx.handle, C.byref(st))
    return rc, st


def rx_balance_rank(hash32: int, g: int) -> int:
    return int(lib().udpdk_gpu_rx_balance_rank(hash32, g))


def rx_balance_run(ctx: GpuContext, b: RxDeviceBatch, meta: np.ndarray, lane_off: np.ndarray,
                   lane_pkt: np.ndarray, lane_rp: np.ndarray, *, hashes: np.ndarray | None = None,
                   n: int | None = None, lane_cap: int | None = None, out_cap: int | None = None,
                   pad: int = 0, fill: int = 0xA5A5A5A5):
    """udpdk_gpu_rx_balance_select over host lane arrays and a device batch: upload, run, download;
    rx_filter_run's conventions. Returns (lane_off_out, lane_pkt_out[out_cap + pad],
    RxBalanceStats, rc of udpdk_gpu_rx_balance_stats)."""
    meta = np.ascontiguousarray(meta, np.uint32)
    lane_off = np.ascontiguousarray(lane_off, np.uint32)
    lane_pkt = np.ascontiguousarray(lane_pkt, np.uint32)
    lane_rp = np.ascontiguousarray(lane_rp, np.uint8)
    n = len(meta) if n is None else n
    lane_cap = len(lane_pkt) if lane_cap is None else lane_cap
    out_cap = lane_cap if out_cap is None else out_cap
    n_lanes = len(lane_off) - 1
    bufs = [ctx.upload(meta), ctx.upload(lane_off), ctx.upload(lane_pkt), ctx.upload(lane_rp),
            ctx.upload(np.full(n_lanes + 1, fill, np.uint32)),
            ctx.upload(np.full(out_cap + pad, fill, np.uint32))]
    if hashes is not None:
        bufs.append(ctx.upload(np.ascontiguousarray(hashes, np.uint32)))
    md, od, pd, rd, oo, po = bufs[:6]
    try:
        bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                     b.ptype.ptr if b.ptype is not None else None, n)
        lanes = RxLanes(md.ptr, n, od.ptr, pd.ptr, lane_cap, n_lanes)
        _check(lib().udpdk_gpu_rx_balance_select(
            ctx.handle, C.byref(bt), C.byref(lanes), C.c_void_p(rd.ptr),
            C.c_void_p(bufs[6].ptr) if hashes is not None else None, C.c_void_p(oo.ptr),
            C.c_void_p(po.ptr), out_cap), "udpdk_gpu_rx_balance_select")
        rc, st = rx_balance_stats(ctx)
        return (ctx.download(oo, np.uint32, n_lanes + 1), ctx.download(po, np.uint32, out_cap + pad),
                st, rc)
    finally:
        for x in bufs:
            x.free()


def rx_peer_stats(ctx: GpuContext) -> tuple[int, RxPeerStats]:
    st = RxPeerStats()
    rc = lib().udpdk_gpu_rx_peer_stats(ctx.handle, C.byref(st))
    return rc, st


def rx_peer_run(ctx: GpuContext, b: RxDeviceBatch, lane_off: np.ndarray, lane_pkt: np.ndarray,
                peers: np.ndarray, *, n: int | None = None, lane_cap: int | None = None,
                out_cap: int | None = None, pad: int = 0, fill: int = 0xA5A5A5A5):
    """udpdk_gpu_rx_peer_select over host lane arrays and a device batch: upload, run, download;
    rx_filter_run's conventions (no verdict words: the stage reads none). Returns (lane_off_out,
    lane_pkt_out[out_cap + pad], RxPeerStats, rc of udpdk_gpu_rx_peer_stats)."""
    lane_off = np.ascontiguousarray(lane_off, np.uint32)
    lane_pkt = np.ascontiguousarray(lane_pkt, np.uint32)
    peers = np.ascontiguousarray(peers, PEER_DTYPE)
    n = b.n if n is None else n
    lane_cap = len(lane_pkt) if lane_cap is None else lane_cap
    out_cap = lane_cap if out_cap is None else out_cap
    n_lanes = len(lane_off) - 1
    bufs = [ctx.upload(lane_off), ctx.upload(lane_pkt), ctx.upload(peers.view(np.uint8)),
            ctx.upload(np.full(n_lanes + 1, fill, np.uint32)),
            ctx.upload(np.full(out_cap + pad, fill, np.uint32))]
    od, pd, rd, oo, po = bufs
    try:
        bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                     b.ptype.ptr if b.ptype is not None else None, n)
        lanes = RxLanes(None, n, od.ptr, pd.ptr, lane_cap, n_lanes)
        _check(lib().udpdk_gpu_rx_peer_select(ctx.handle, C.byref(bt), C.byref(lanes), C.c_void_p(rd.ptr),
                                              C.c_void_p(oo.ptr), C.c_void_p(po.ptr), out_cap),
               "udpdk_gpu_rx_peer_select")
        rc, st = rx_peer_stats(ctx)
        return (ctx.download(oo, np.uint32, n_lanes + 1), ctx.download(po, np.uint32, out_cap + pad),
                st, rc)
    finally:
        for x in bufs:
            x.free()


def mcast_table_build(members, slots: int) -> tuple[int, np.ndarray]:
    """udpdk_gpu_mcast_table_build: (rc, table[slots] as MCAST_DTYPE; 0xA5 bytes where the call
    wrote nothing). Host only."""
    m = np.ascontiguousarray(members, MCAST_DTYPE)
    tab = np.full(8 * max(1, min(slots, MCAST_MAX_SLOTS)), 0xA5, np.uint8).view(MCAST_DTYPE)
    rc = lib().udpdk_gpu_mcast_table_build(m.ctypes.data_as(C.c_void_p) if len(m) else None, len(m),
                                           tab.ctypes.data_as(C.c_void_p), slots)
    return rc, tab


def rx_mcast_stats(ctx: GpuContext) -> tuple[int, RxMcastStats]:
    st = RxMcastStats()
    rc = lib().udpdk_gpu_rx_mcast_stats(ctx.handle, C.byref(st))
    return rc, st


def rx_mcast_run(ctx: GpuContext, b: RxDeviceBatch, lane_off: np.ndarray, lane_pkt: np.ndarray,
                 lane_mc: np.ndarray, table: np.ndarray, *, n: int | None = None, lane_cap: int | None = None,
                 out_cap: int | None = None, pad: int = 0, fill: int = 0xA5A5A5A5):
    """udpdk_gpu_rx_mcast_select over host lane arrays, a table (MCAST_DTYPE[slots]) and a device
    batch: upload, run, download; rx_peer_run's conventions. Returns (lane_off_out,
    lane_pkt_out[out_cap + pad], RxMcastStats, rc of udpdk_gpu_rx_mcast_stats)."""
    lane_off = np.ascontiguousarray(lane_off, np.uint32)
    lane_pkt = np.ascontiguousarray(lane_pkt, np.uint32)
    lane_mc = np.ascontiguousarray(lane_mc, np.uint8)
    table = np.ascontiguousarray(table, MCAST_DTYPE)
    n = b.n if n is None else n
    lane_cap = len(lane_pkt) if lane_cap is None else lane_cap
    out_cap = lane_cap if out_cap is None else out_cap
    n_lanes = len(lane_off) - 1
    assert len(lane_mc) >= n_lanes
    bufs = [ctx.upload(lane_off), ctx.upload(lane_pkt), ctx.upload(lane_mc), ctx.upload(table.view(np.uint8)),
            ctx.upload(np.full(n_lanes + 1, fill, np.uint32)),
            ctx.upload(np.full(out_cap + pad, fill, np.uint32))]
    od, pd, md, td, oo, po = bufs
    try:
        bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                     b.ptype.ptr if b.ptype is not None else None, n)
        lanes = RxLanes(None, n, od.ptr, pd.ptr, lane_cap, n_lanes)
        _check(lib().udpdk_gpu_rx_mcast_select(ctx.handle, C.byref(bt), C.byref(lanes), C.c_void_p(md.ptr),
                                               C.c_void_p(td.ptr), len(table), C.c_void_p(oo.ptr),
                                               C.c_void_p(po.ptr), out_cap),
               "udpdk_gpu_rx_mcast_select")
        rc, st = rx_mcast_stats(ctx)
        return (ctx.download(oo, np.uint32, n_lanes + 1), ctx.download(po, np.uint32, out_cap + pad),
                st, rc)
    finally:
        for x in bufs:
            x.free()


@dataclass
class RxDeviceGather:
    payload: DeviceBuffer
    slot_bytes: int
    length: DeviceBuffer
    src_ip: DeviceBuffer
    src_port: DeviceBuffer
    count: int


def rx_alloc_gather(ctx: GpuContext, count: int, slot_bytes: int) -> RxDeviceGather:
    c = max(1, count)
    return RxDeviceGather(ctx.alloc(c * slot_bytes), slot_bytes, ctx.alloc(4 * c), ctx.alloc(4 * c),
                          ctx.alloc(2 * c), count)


def rx_gather_enqueue(ctx: GpuContext, b: RxDeviceBatch, lane_pkt: DeviceBuffer, first: int,
                      g: RxDeviceGather) -> int:
    bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                 b.ptype.ptr if b.ptype is not None else None, b.n)
    gt = RxGather(g.payload.ptr, g.slot_bytes, g.length.ptr, g.src_ip.ptr, g.src_port.ptr)
    return lib().udpdk_gpu_rx_gather(ctx.handle, C.byref(bt), C.c_void_p(lane_pkt.ptr), first,
                                     g.count, C.byref(gt))


def rx_gather_run(ctx: GpuContext, b: RxDeviceBatch, lane_pkt: DeviceBuffer, first: int,
                  g: RxDeviceGather):
    """Gather lane entries [first, first + count) and download (payload slots as a
    [count, slot_bytes] u8 array, len, src_ip, src_port)."""
    _check(rx_gather_enqueue(ctx, b, lane_pkt, first, g), "udpdk_gpu_rx_gather")
    ctx.sync()
    pay = ctx.download(g.payload, np.uint8, g.count * g.slot_bytes).reshape(g.count, g.slot_bytes)
    return (pay, ctx.download(g.length, np.uint32, g.count), ctx.download(g.src_ip, np.uint32, g.count),
            ctx.download(g.src_port, np.uint16, g.count))


def rx_gather_packed_run(ctx: GpuContext, b: RxDeviceBatch, lane_pkt: DeviceBuffer, first: int,
                         slot_off: np.ndarray):
    """udpdk_gpu_rx_gather_packed over lane entries [first, first + len(slot_off) - 1): entry k's
    buffer is bytes [slot_off[k], slot_off[k + 1]) of one payload area. Returns (payload area
    u8, len, src_ip, src_port)."""
    count = len(slot_off) - 1
    so = ctx.upload(np.asarray(slot_off, np.uint32))
    total = int(slot_off[-1])
    pay = ctx.alloc(max(16, total))
    ln, ip, pt = ctx.alloc(4 * max(1, count)), ctx.alloc(4 * max(1, count)), ctx.alloc(2 * max(1, count))
    bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                 b.ptype.ptr if b.ptype is not None else None, b.n)
    gt = RxGather(pay.ptr, 16, ln.ptr, ip.ptr, pt.ptr)
    _check(lib().udpdk_gpu_rx_gather_packed(ctx.handle, C.byref(bt), C.c_void_p(lane_pkt.ptr), first, count,
                                            C.c_void_p(so.ptr), C.byref(gt)), "udpdk_gpu_rx_gather_packed")
    ctx.sync()
    out = (ctx.download(pay, np.uint8, total), ctx.download(ln, np.uint32, count),
           ctx.download(ip, np.uint32, count), ctx.download(pt, np.uint16, count))
    for x in (so, pay, ln, ip, pt):
        x.free()
    return out


def tx_reply_geometry(count: int) -> tuple[int, int]:
    """(entries per workgroup, workgroups) of the reply plan kernels for `count` entries."""
    e = C.c_uint32()
    k = C.c_uint32()
    _check(lib().udpdk_gpu_tx_reply_geometry(count, C.byref(e), C.byref(k)), "udpdk_gpu_tx_reply_geometry")
    return e.value, k.value


def tx_reply_stats(ctx: GpuContext) -> tuple[int, TxReplyStats]:
    st = TxReplyStats()
    rc = lib().udpdk_gpu_tx_reply_stats(ctx.handle, C.byref(st))
    return rc, st


PLAN_FIELDS = (("payload_off", np.uint32), ("payload_len", np.uint16), ("sockfd", np.int32),
               ("dst_ip", np.uint32), ("dst_port", np.uint16), ("frame_off", np.uint32))


def _tx_reply(ctx: GpuContext, cfg, b: RxDeviceBatch, lane_off, lane_pkt, first: int, count: int, *,
              mtu: int, flags: int, out_cap: int, lane_sel, lane_cap, n, n_lanes, pad: int, guard: int,
              out_ptr):
    lane_off = np.ascontiguousarray(lane_off, np.uint32)
    lane_pkt = np.ascontiguousarray(lane_pkt, np.uint32)
    n_lanes = len(lane_off) - 1 if n_lanes is None else n_lanes
    lane_cap = len(lane_pkt) if lane_cap is None else lane_cap
    bufs = [ctx.upload(lane_off), ctx.upload(lane_pkt)]
    sel = None
    if lane_sel is not None:
        sel = ctx.upload(np.ascontiguousarray(lane_sel, np.uint8))
        bufs.append(sel)
    # the plan arrays, `pad` elements longer than the call may write, every byte 0xA5
    arrs = []
    for name, dt in PLAN_FIELDS:
        m = count + pad + (1 if name == "frame_off" else 0)
        arrs.append(ctx.upload(np.full(max(1, m) * np.dtype(dt).itemsize, 0xA5, np.uint8)))
    out = None
    if cfg is not None and out_ptr is None:
        out = ctx.upload(np.full(out_cap + guard, 0xEE, np.uint8))
    bufs += arrs + ([out] if out is not None else [])
    try:
        bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                     b.ptype.ptr if b.ptype is not None else None, b.n if n is None else n)
        lanes = RxLanes(None, bt.n, bufs[0].ptr, bufs[1].ptr, lane_cap, n_lanes)
        plan = TxReplyPlan(*[a.ptr for a in arrs])
        selp = C.c_void_p(sel.ptr) if sel is not None else None
        if cfg is None:
            rc = lib().udpdk_gpu_tx_reply_plan(ctx.handle, C.byref(bt), C.byref(lanes), first, count, selp,
                                               mtu, out_cap, C.byref(plan))
        else:
            rc = lib().udpdk_gpu_tx_reply(ctx.handle, C.byref(cfg), C.byref(bt), C.byref(lanes), first, count,
                                          selp, mtu, flags, C.c_void_p(out.ptr if out is not None else out_ptr),
                                          out_cap, C.byref(plan))
        ctx.sync()
        res = {"rc": rc}
        for (name, dt), a in zip(PLAN_FIELDS, arrs):
            res[name] = ctx.download(a, dt, count + pad + (1 if name == "frame_off" else 0))
        if out is not None:
            res["out"] = ctx.download(out, np.uint8, out_cap + guard)
        return res
    finally:
        for x in bufs:
            x.free()


def tx_reply_plan_run(ctx: GpuContext, b: RxDeviceBatch, lane_off, lane_pkt, first: int, count: int, *,
                      mtu: int = 0, out_cap: int = 1 << 24, lane_sel=None, lane_cap=None, n=None,
                      n_lanes=None, pad: int = 8):
    """udpdk_gpu_tx_reply_plan over host lanes (uploaded whole; lane_cap defaults to len(lane_pkt),
    n_lanes to len(lane_off) - 1, n to the batch's). Returns a dict: rc of the call and the six plan
    arrays as downloaded, each `pad` elements longer than the call may write and pre-filled with
    0xA5 bytes. The snapshot with the slot table must have been uploaded."""
    return _tx_reply(ctx, None, b, lane_off, lane_pkt, first, count, mtu=mtu, flags=0, out_cap=out_cap,
                     lane_sel=lane_sel, lane_cap=lane_cap, n=n, n_lanes=n_lanes, pad=pad, guard=0, out_ptr=None)


def tx_reply_run(ctx: GpuContext, cfg: TxConfig, b: RxDeviceBatch, lane_off, lane_pkt, first: int, count: int, *,
                 mtu: int = 0, flags: int = 0, out_cap: int = 1 << 20, lane_sel=None, lane_cap=None, n=None,
                 n_lanes=None, pad: int = 8, guard: int = 4096, out_ptr=None):
    """udpdk_gpu_tx_reply the same way; res["out"] is the output buffer, out_cap + guard bytes
    pre-filled with 0xEE (out_ptr: a caller's device pointer instead, nothing downloaded)."""
    return _tx_reply(ctx, cfg, b, lane_off, lane_pkt, first, count, mtu=mtu, flags=flags, out_cap=out_cap,
                     lane_sel=lane_sel, lane_cap=lane_cap, n=n, n_lanes=n_lanes, pad=pad, guard=guard,
                     out_ptr=out_ptr)


def tx_segment_span(length: int, gso: int, mtu: int) -> tuple[int, int, int]:
    """udpdk_gpu_tx_segment_span: (output bytes, segments, frames) of one send (host only)."""
    ns, nf = C.c_uint32(), C.c_uint32()
    span = lib().udpdk_gpu_tx_segment_span(length, gso, mtu, C.byref(ns), C.byref(nf))
    return int(span), ns.value, nf.value


def tx_segment_geometry(k: int, max_segs: int) -> tuple[int, int, int, int]:
    """(sends per workgroup, segments per workgroup, send workgroups, segment workgroups) of the
    segment plan kernels."""
    v = [C.c_uint32() for _ in range(4)]
    _check(lib().udpdk_gpu_tx_segment_geometry(k, max_segs, *[C.byref(x) for x in v]), "udpdk_gpu_tx_segment_geometry")
    return tuple(x.value for x in v)


def tx_segment_stats(ctx: GpuContext) -> tuple[int, TxSegmentStats]:
    st = TxSegmentStats()
    rc = lib().udpdk_gpu_tx_segment_stats(ctx.handle, C.byref(st))
    return rc, st


SEND_FIELDS = (("payload_off", np.uint32), ("payload_len", np.uint16), ("gso_size", np.uint16), ("sockfd", np.int32),
               ("dst_ip", np.uint32), ("dst_port", np.uint16))


def _tx_segment(ctx: GpuContext, cfg, payload: np.ndarray, payload_bytes: int, sends: dict, max_segs: int, *, mtu: int,
                flags: int, seg_limit: int, out_cap: int, k, pad: int, guard: int, null=None):
    ka = len(sends["payload_off"])                    # what is allocated; k: what the call is told
    k = ka if k is None else k
    bufs = [ctx.upload(np.ascontiguousarray(payload, np.uint8))]
    ins = [ctx.upload(np.ascontiguousarray(sends[name], dt) if len(sends[name]) else np.zeros(1, dt))
           for name, dt in SEND_FIELDS]
    # the plan arrays, `pad` elements longer than the call may write, every byte 0xA5
    arrs = []
    for name, dt in PLAN_FIELDS + (("seg_off", np.uint32),):
        m = (ka + 1 if name == "seg_off" else max_segs + (1 if name == "frame_off" else 0)) + pad
        arrs.append(ctx.upload(np.full(max(1, m) * np.dtype(dt).itemsize, 0xA5, np.uint8)))
    out = ctx.upload(np.full(out_cap + guard, 0xEE, np.uint8)) if cfg is not None else None
    bufs += ins + arrs + ([out] if out is not None else [])
    try:
        sd = TxSends(bufs[0].ptr, payload_bytes, *[x.ptr for x in ins], k)
        plan = TxSegmentPlan(*[a.ptr for a in arrs], max_segs)
        if null is not None:                          # ("sends" | "plan", field): that pointer is NULL
            setattr(sd if null[0] == "sends" else plan, null[1], None)
        if cfg is None:
            rc = lib().udpdk_gpu_tx_segment_plan(ctx.handle, C.byref(sd), mtu, seg_limit, out_cap, C.byref(plan))
        else:
            rc = lib().udpdk_gpu_tx_segment(ctx.handle, C.byref(cfg), C.byref(sd), mtu, flags, seg_limit,
                                            C.c_void_p(out.ptr), out_cap, C.byref(plan))
        ctx.sync()
        res = {"rc": rc}
        for (name, dt), a in zip(PLAN_FIELDS + (("seg_off", np.uint32),), arrs):
            m = (ka + 1 if name == "seg_off" else max_segs + (1 if name == "frame_off" else 0)) + pad
            res[name] = ctx.download(a, dt, m)
        if out is not None:
            res["out"] = ctx.download(out, np.uint8, out_cap + guard)
        return res
    finally:
        for x in bufs:
            x.free()


def tx_segment_plan_run(ctx: GpuContext, payload: np.ndarray, payload_bytes: int, sends: dict, max_segs: int, *,
                        mtu: int = 0, seg_limit: int = 0, out_cap: int = 1 << 24, k=None, pad: int = 8, null=None):
    """udpdk_gpu_tx_segment_plan over host sends: a dict of the six SEND_FIELDS arrays, against
    `payload` (uploaded whole, tailroom included; payload_bytes is what the call is told). Returns a
    dict: rc of the call, the six plan arrays and seg_off as downloaded, each `pad` elements longer
    than the call may write and pre-filled with 0xA5 bytes. null = ("sends" | "plan", field) passes that
    pointer as NULL."""
    return _tx_segment(ctx, None, payload, payload_bytes, sends, max_segs, mtu=mtu, flags=0, seg_limit=seg_limit,
                       out_cap=out_cap, k=k, pad=pad, guard=0, null=null)


def tx_segment_run(ctx: GpuContext, cfg: TxConfig, payload: np.ndarray, payload_bytes: int, sends: dict,
                   max_segs: int, *, mtu: int = 0, flags: int = 0, seg_limit: int = 0, out_cap: int = 1 << 20, k=None,
                   pad: int = 8, guard: int = 4096):
    """udpdk_gpu_tx_segment the same way; res["out"] is the output buffer, out_cap + guard bytes
    pre-filled with 0xEE. The snapshot with the slot table must have been uploaded."""
    return _tx_segment(ctx, cfg, payload, payload_bytes, sends, max_segs, mtu=mtu, flags=flags, seg_limit=seg_limit,
                       out_cap=out_cap, k=k, pad=pad, guard=guard)


def icmp_geometry(n: int) -> tuple[int, int]:
    """(frames per workgroup, workgroups) of the ICMP scan and build kernels for n frames."""
    e = C.c_uint32()
    k = C.c_uint32()
    _check(lib().udpdk_gpu_icmp_geometry(n, C.byref(e), C.byref(k)), "udpdk_gpu_icmp_geometry")
    return e.value, k.value


def icmp_run(ctx: GpuContext, cfg: TxConfig, b: RxDeviceBatch, meta, *, flags: int = ICMP_ALL, mtu: int = 0,
             err_limit: int = 0xFFFFFFFF, out_cap: int = 1 << 20, max_replies=None, n=None, pipe: int = 0,
             pad: int = 8, guard: int = 4096):
    """udpdk_gpu_icmp_reply (pipe 0) or udpdk_gpu_pipe_icmp_reply + udpdk_gpu_pipe_wait over host verdict
    words. Returns a dict: rc of the call, rc and struct of the stats call, reply_off and origin as
    downloaded (`pad` elements longer than the call may write, pre-filled with 0xA5 bytes) and out:
    out_cap + guard bytes pre-filled with 0xEE."""
    meta = np.ascontiguousarray(meta, np.uint32)
    n = b.n if n is None else n
    max_replies = n if max_replies is None else max_replies
    bufs = [ctx.upload(meta), ctx.upload(np.full(4 * (max_replies + 1 + pad), 0xA5, np.uint8)),
            ctx.upload(np.full(4 * (max_replies + pad), 0xA5, np.uint8)),
            ctx.upload(np.full(out_cap + guard, 0xEE, np.uint8))]
    try:
        bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                     b.ptype.ptr if b.ptype is not None else None, n)
        o = IcmpOut(bufs[3].ptr, out_cap, bufs[1].ptr, bufs[2].ptr, max_replies)
        st = IcmpStats()
        if pipe:
            rc = lib().udpdk_gpu_pipe_icmp_reply(ctx.handle, pipe, C.byref(cfg), C.byref(bt), C.c_void_p(bufs[0].ptr),
                                                 flags, mtu, err_limit, C.byref(o))
            _check(lib().udpdk_gpu_pipe_wait(ctx.handle, pipe), "udpdk_gpu_pipe_wait")
            src = lib().udpdk_gpu_pipe_icmp_stats(ctx.handle, pipe, C.byref(st))
        else:
            rc = lib().udpdk_gpu_icmp_reply(ctx.handle, C.byref(cfg), C.byref(bt), C.c_void_p(bufs[0].ptr), flags,
                                            mtu, err_limit, C.byref(o))
            src = lib().udpdk_gpu_icmp_stats(ctx.handle, C.byref(st))
        ctx.sync()
        return {"rc": rc, "stats_rc": src, "stats": st,
                "reply_off": ctx.download(bufs[1], np.uint32, max_replies + 1 + pad),
                "origin": ctx.download(bufs[2], np.uint32, max_replies + pad),
                "out": ctx.download(bufs[3], np.uint8, out_cap + guard)}
    finally:
        for x in bufs:
            x.free()


def arp_geometry(n: int) -> tuple[int, int]:
    """(frames per workgroup, workgroups) of the ARP kernel for n frames."""
    e = C.c_uint32()
    k = C.c_uint32()
    _check(lib().udpdk_gpu_arp_geometry(n, C.byref(e), C.byref(k)), "udpdk_gpu_arp_geometry")
    return e.value, k.value


def arp_run(ctx: GpuContext, cfg: TxConfig, b: RxDeviceBatch, meta, *, max_replies=None, n=None, pipe: int = 0,
            pad: int = 8):
    """udpdk_gpu_arp_reply (pipe 0) or udpdk_gpu_pipe_arp_reply + udpdk_gpu_pipe_wait over host verdict
    words. Returns a dict: rc of the call, rc and dict of the stats call, meta as downloaded afterwards,
    and slots [max_replies + pad, 64] and origin [max_replies + pad] as downloaded, `pad` elements longer
    than the call may write and pre-filled with 0xA5 bytes."""
    meta = np.ascontiguousarray(meta, np.uint32)
    n = b.n if n is None else n
    max_replies = n if max_replies is None else max_replies
    bufs = [ctx.upload(meta if meta.size else np.zeros(1, np.uint32)),
            ctx.upload(np.full(ARP_SLOT_BYTES * (max_replies + pad), 0xA5, np.uint8)),
            ctx.upload(np.full(4 * (max_replies + pad), 0xA5, np.uint8))]
    try:
        bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                     b.ptype.ptr if b.ptype is not None else None, n)
        o = ArpOut(bufs[1].ptr, bufs[2].ptr, max_replies)
        st = ArpStats()
        if pipe:
            rc = lib().udpdk_gpu_pipe_arp_reply(ctx.handle, pipe, C.byref(cfg), C.byref(bt), C.c_void_p(bufs[0].ptr),
                                                C.byref(o))
            _check(lib().udpdk_gpu_pipe_wait(ctx.handle, pipe), "udpdk_gpu_pipe_wait")
            src = lib().udpdk_gpu_pipe_arp_stats(ctx.handle, pipe, C.byref(st))
        else:
            rc = lib().udpdk_gpu_arp_reply(ctx.handle, C.byref(cfg), C.byref(bt), C.c_void_p(bufs[0].ptr), C.byref(o))
            src = lib().udpdk_gpu_arp_stats(ctx.handle, C.byref(st))
        ctx.sync()
        return {"rc": rc, "stats_rc": src, "stats": {k: getattr(st, k) for k in ARP_STATS},
                "meta": ctx.download(bufs[0], np.uint32, max(1, meta.size))[:meta.size],
                "slots": ctx.download(bufs[1], np.uint8, ARP_SLOT_BYTES * (max_replies + pad)).reshape(-1, ARP_SLOT_BYTES),
                "origin": ctx.download(bufs[2], np.uint32, max_replies + pad)}
    finally:
        for x in bufs:
            x.free()


def igmp_geometry(n: int) -> tuple[int, int]:
    """(frames per workgroup, workgroups) of the IGMP kernel for n frames."""
    e = C.c_uint32()
    k = C.c_uint32()
    _check(lib().udpdk_gpu_igmp_geometry(n, C.byref(e), C.byref(k)), "udpdk_gpu_igmp_geometry")
    return e.value, k.value


def igmp_run(ctx: GpuContext, cfg: TxConfig, b: RxDeviceBatch, meta, groups, *, max_reports=None, n=None,
             pipe: int = 0, pad: int = 8):
    """udpdk_gpu_igmp_reply (pipe 0) or udpdk_gpu_pipe_igmp_reply + udpdk_gpu_pipe_wait over host verdict
    words and raw group addresses. Returns a dict: rc of the call, rc and dict of the stats call, and
    slots [max_reports + pad, 64] and group_index [max_reports + pad] as downloaded, `pad` elements
    longer than the call may write and pre-filled with 0xA5 bytes."""
    meta = np.ascontiguousarray(meta, np.uint32)
    groups = np.ascontiguousarray(groups, np.uint32)
    n = b.n if n is None else n
    max_reports = len(groups) if max_reports is None else max_reports
    bufs = [ctx.upload(meta if meta.size else np.zeros(1, np.uint32)),
            ctx.upload(groups if groups.size else np.zeros(1, np.uint32)),
            ctx.upload(np.full(IGMP_SLOT_BYTES * (max_reports + pad), 0xA5, np.uint8)),
            ctx.upload(np.full(4 * (max_reports + pad), 0xA5, np.uint8))]
    try:
        bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                     b.ptype.ptr if b.ptype is not None else None, n)
        o = IgmpOut(bufs[2].ptr, bufs[3].ptr, max_reports)
        st = IgmpStats()
        args = (C.byref(cfg), C.byref(bt), C.c_void_p(bufs[0].ptr), C.c_void_p(bufs[1].ptr), len(groups), C.byref(o))
        if pipe:
            rc = lib().udpdk_gpu_pipe_igmp_reply(ctx.handle, pipe, *args)
            _check(lib().udpdk_gpu_pipe_wait(ctx.handle, pipe), "udpdk_gpu_pipe_wait")
            src = lib().udpdk_gpu_pipe_igmp_stats(ctx.handle, pipe, C.byref(st))
        else:
            rc = lib().udpdk_gpu_igmp_reply(ctx.handle, *args)
            src = lib().udpdk_gpu_igmp_stats(ctx.handle, C.byref(st))
        ctx.sync()
        return {"rc": rc, "stats_rc": src, "stats": {k: getattr(st, k) for k in IGMP_STATS},
                "slots": ctx.download(bufs[2], np.uint8, IGMP_SLOT_BYTES * (max_reports + pad)).reshape(-1, IGMP_SLOT_BYTES),
                "group_index": ctx.download(bufs[3], np.uint32, max_reports + pad)}
    finally:
        for x in bufs:
            x.free()


def neigh_cfg(src_ip: str | int, src_mac: bytes, *, netmask: str | int = 0, gateway: str | int = 0,
              fallback_mac: bytes = bytes(6), ttl_ms: int = 30000, retrans_ms: int = 1000, flags: int = 0) -> NeighCfg:
    """A udpdk_neigh_cfg_t; addresses as dotted strings or raw."""
    raw = lambda a: raw_ip(a) if isinstance(a, str) else int(a)
    return NeighCfg(raw(src_ip), raw(netmask), raw(gateway), (C.c_uint8 * 6)(*src_mac), (C.c_uint8 * 6)(*fallback_mac),
                    ttl_ms, retrans_ms, flags)


def neigh_geometry() -> tuple[int, int]:
    """(frames per workgroup of the learn kernel, datagrams per workgroup of the resolve kernel)."""
    t = C.c_uint32()
    b = C.c_uint32()
    _check(lib().udpdk_gpu_neigh_geometry(C.byref(t), C.byref(b)), "udpdk_gpu_neigh_geometry")
    return t.value, b.value


def neigh_class(cfg: NeighCfg, dst_ip: int) -> tuple[int, int, bytes]:
    """udpdk_gpu_neigh_class: (class, next hop, MAC)."""
    h = C.c_uint32(0xDEADBEEF)
    mac = (C.c_uint8 * 6)(*([0xA5] * 6))
    return lib().udpdk_gpu_neigh_class(C.byref(cfg), dst_ip, C.byref(h), mac), h.value, bytes(mac)


def neigh_create(ctx: GpuContext, entries: int) -> int:
    return lib().udpdk_gpu_neigh_create(ctx.handle, entries)


def neigh_set(ctx: GpuContext, entries) -> int:
    """entries: (raw ip, mac bytes, state, stamp) tuples."""
    arr = (NeighEntry * max(1, len(entries)))()
    for e, (ip, mac, state, stamp) in zip(arr, entries):
        e.ip, e.mac, e.state, e.stamp = ip, (C.c_uint8 * 6)(*mac), state, stamp
    return lib().udpdk_gpu_neigh_set(ctx.handle, arr, len(entries))


def neigh_dump(ctx: GpuContext, cap: int = NEIGH_MAX_ENTRIES, as_list: bool = False):
    """The table as a map: raw ip -> (mac, state, stamp); as_list: (ip, mac, state, stamp) in the table's order."""
    arr = (NeighEntry * max(1, cap))()
    n = C.c_uint32()
    _check(lib().udpdk_gpu_neigh_dump(ctx.handle, arr, cap, C.byref(n)), "udpdk_gpu_neigh_dump")
    if as_list:
        return [(e.ip, bytes(e.mac), e.state, e.stamp) for e in arr[:n.value]]
    return {e.ip: (bytes(e.mac), e.state, e.stamp) for e in arr[:n.value]}


def neigh_flush(ctx: GpuContext, keep_static: bool = False) -> int:
    return lib().udpdk_gpu_neigh_flush(ctx.handle, int(keep_static))


def neigh_learn_run(ctx: GpuContext, cfg: NeighCfg, b: RxDeviceBatch, meta, now: int, *, n=None, pipe: int = 0):
    """udpdk_gpu_neigh_learn (pipe 0) or udpdk_gpu_pipe_neigh_learn + udpdk_gpu_pipe_wait over host verdict
    words. Returns a dict: rc of the call, rc and dict of the stats call, meta as downloaded afterwards."""
    meta = np.ascontiguousarray(meta, np.uint32)
    n = b.n if n is None else n
    buf = ctx.upload(meta if meta.size else np.zeros(1, np.uint32))
    try:
        bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                     b.ptype.ptr if b.ptype is not None else None, n)
        st = NeighLearnStats()
        if pipe:
            rc = lib().udpdk_gpu_pipe_neigh_learn(ctx.handle, pipe, C.byref(cfg), C.byref(bt), C.c_void_p(buf.ptr), now)
            _check(lib().udpdk_gpu_pipe_wait(ctx.handle, pipe), "udpdk_gpu_pipe_wait")
            src = lib().udpdk_gpu_pipe_neigh_learn_stats(ctx.handle, pipe, C.byref(st))
        else:
            rc = lib().udpdk_gpu_neigh_learn(ctx.handle, C.byref(cfg), C.byref(bt), C.c_void_p(buf.ptr), now)
            src = lib().udpdk_gpu_neigh_learn_stats(ctx.handle, C.byref(st))
        ctx.sync()
        return {"rc": rc, "stats_rc": src, "stats": {k: getattr(st, k) for k in NEIGH_LEARN_STATS},
                "meta": ctx.download(buf, np.uint32, max(1, meta.size))[:meta.size]}
    finally:
        buf.free()


def neigh_resolve_run(ctx: GpuContext, cfg: NeighCfg, dst_ip, sockfd, now: int, *, req_cap=None, pad: int = 4):
    """udpdk_gpu_neigh_resolve over host arrays. Returns a dict: rc of the call, rc and dict of the stats
    call, dmac [n + pad, 2], sockfd_out, state, req [req_cap + pad, 64] and req_origin as downloaded, each `pad`
    elements longer than the call may write and pre-filled with 0xA5 bytes, and dst_ip and sockfd as
    downloaded afterwards."""
    dst_ip = np.ascontiguousarray(dst_ip, np.uint32)
    sockfd = np.ascontiguousarray(sockfd, np.int32)
    n = dst_ip.size
    req_cap = n if req_cap is None else req_cap
    can = lambda nbytes: ctx.upload(np.full(max(nbytes, 16), 0xA5, np.uint8))
    bufs = [ctx.upload(dst_ip if n else np.zeros(1, np.uint32)), ctx.upload(sockfd if n else np.zeros(1, np.int32)),
            can(8 * (n + pad)), can(4 * (n + pad)), can(n + pad), can(ARP_SLOT_BYTES * (req_cap + pad)),
            can(4 * (req_cap + pad))]
    try:
        o = NeighOut(bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, bufs[6].ptr, req_cap)
        st = NeighResolveStats()
        rc = lib().udpdk_gpu_neigh_resolve(ctx.handle, C.byref(cfg), C.c_void_p(bufs[0].ptr), C.c_void_p(bufs[1].ptr), n,
                                           now, C.byref(o))
        src = lib().udpdk_gpu_neigh_resolve_stats(ctx.handle, C.byref(st))
        ctx.sync()
        return {"rc": rc, "stats_rc": src, "stats": {k: getattr(st, k) for k in NEIGH_RESOLVE_STATS},
                "dmac": ctx.download(bufs[2], np.uint32, 2 * (n + pad)).reshape(-1, 2),
                "sockfd_out": ctx.download(bufs[3], np.int32, n + pad),
                "state": ctx.download(bufs[4], np.uint8, n + pad),
                "req": ctx.download(bufs[5], np.uint8, ARP_SLOT_BYTES * (req_cap + pad)).reshape(-1, ARP_SLOT_BYTES),
                "req_origin": ctx.download(bufs[6], np.uint32, req_cap + pad),
                "dst_ip": ctx.download(bufs[0], np.uint32, max(1, n))[:n],
                "sockfd": ctx.download(bufs[1], np.int32, max(1, n))[:n]}
    finally:
        for x in bufs:
            x.free()


def icmp_errno(code: int) -> tuple[int, int]:
    """udpdk_gpu_icmp_errno: (errno, hard) of a destination-unreachable code."""
    h = C.c_int(-1)
    return lib().udpdk_gpu_icmp_errno(code, C.byref(h)), h.value


def icmp_err_run(ctx: GpuContext, our_ip: int, b: RxDeviceBatch, meta, peers, n_lanes: int, *, n=None,
                 pipe: int = 0, pad: int = 8, err_ptr=None, peer_ptr=None):
    """udpdk_gpu_icmp_errors (pipe 0) or udpdk_gpu_pipe_icmp_errors + udpdk_gpu_pipe_wait over host verdict
    words. peers: PEER_DTYPE records uploaded as peer_dev, or None for the context's sticky table.
    Returns a dict: rc of the call, rc and struct of the stats call, and err: the words as downloaded,
    `pad` longer than the call may write and pre-filled with 0xA5 bytes. err_ptr / peer_ptr replace
    the device pointers (argument checks)."""
    meta = np.ascontiguousarray(meta, np.uint32)
    n = b.n if n is None else n
    bufs = [ctx.upload(meta), ctx.upload(np.full(8 * (n_lanes + pad), 0xA5, np.uint8))]
    if peers is not None:
        bufs.append(ctx.upload(np.ascontiguousarray(peers, PEER_DTYPE).view(np.uint8)))
    try:
        bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                     b.ptype.ptr if b.ptype is not None else None, n)
        pp = C.c_void_p(peer_ptr if peer_ptr is not None else (bufs[2].ptr if peers is not None else None))
        ep = C.c_void_p(bufs[1].ptr if err_ptr is None else err_ptr)
        st = IcmpErrStats()
        if pipe:
            rc = lib().udpdk_gpu_pipe_icmp_errors(ctx.handle, pipe, our_ip, C.byref(bt), C.c_void_p(bufs[0].ptr), pp,
                                                  n_lanes, ep)
            _check(lib().udpdk_gpu_pipe_wait(ctx.handle, pipe), "udpdk_gpu_pipe_wait")
            src = lib().udpdk_gpu_pipe_icmp_err_stats(ctx.handle, pipe, C.byref(st))
        else:
            rc = lib().udpdk_gpu_icmp_errors(ctx.handle, our_ip, C.byref(bt), C.c_void_p(bufs[0].ptr), pp, n_lanes, ep)
            src = lib().udpdk_gpu_icmp_err_stats(ctx.handle, C.byref(st))
        ctx.sync()
        return {"rc": rc, "stats_rc": src, "stats": {k: getattr(st, k) for k in ICMP_ERR_STATS},
                "err": ctx.download(bufs[1], np.uint64, n_lanes + pad)}
    finally:
        for x in bufs:
            x.free()


@dataclass
class DevRef:
    """A device pointer the context owns (no free)."""
    ptr: int


def frag_table_create(ctx: GpuContext, bucket_num: int = 0x1000, bucket_entries: int = 16,
                      max_cycles: int = 1000, max_dgram: int = 65515, max_entries: int = 0, flags: int = 0):
    cfg = FragTableCfg(bucket_num, bucket_entries, max_cycles, max_dgram, max_entries, flags, 0)
    _check(lib().udpdk_gpu_frag_table_create(ctx.handle, C.byref(cfg)), "udpdk_gpu_frag_table_create")


def rx_reassemble(ctx: GpuContext, b: RxDeviceBatch, meta: DeviceBuffer, tms: int, inplace: bool = False):
    """Reassembly step for a batch whose verdicts are in meta. Returns (RxDeviceBatch of the
    reassembled frames (context-owned, or b's own frame buffer when inplace reassembled every
    datagram in place), origin DevRef, stats dict)."""
    bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                 b.ptype.ptr if b.ptype is not None else None, b.n)
    o = ReasmOut()
    fn = "udpdk_gpu_rx_reassemble_inplace" if inplace else "udpdk_gpu_rx_reassemble"
    _check(getattr(lib(), fn)(ctx.handle, C.byref(bt), C.c_void_p(meta.ptr), tms, C.byref(o)), fn)
    ob = o.batch
    rb = RxDeviceBatch(DevRef(ob.frames_dev or 0), int(ob.frames_bytes), DevRef(ob.offset_dev or 0),
                       DevRef(ob.length_dev or 0), DevRef(ob.ptype_dev or 0), int(ob.n))
    return rb, DevRef(o.origin_dev or 0), dict(zip(RS_STATS, list(o.stats)))


def rss_conf(n_queues: int, reta=None, key: bytes | None = None, hash_types: int = 3) -> RssConf:
    """udpdk_gpu_rss_default_conf, optionally with another redirection table / key / types."""
    cf = RssConf()
    _check(lib().udpdk_gpu_rss_default_conf(C.byref(cf), n_queues), "udpdk_gpu_rss_default_conf")
    if reta is not None:
        cf.reta_size = len(reta)
        for i, q in enumerate(reta):
            cf.reta[i] = int(q)
    if key is not None:
        for i in range(40):
            cf.key[i] = key[i]
    cf.hash_types = hash_types
    return cf


def rss_run(ctx: GpuContext, b: RxDeviceBatch, cf: RssConf):
    """Configure RSS, run it over a device batch and download (hash, queue_off, queue_pkt)."""
    _check(lib().udpdk_gpu_rss_config(ctx.handle, C.byref(cf)), "udpdk_gpu_rss_config")
    n = b.n
    h, qo, qp = ctx.alloc(4 * max(1, n)), ctx.alloc(4 * (cf.n_queues + 1)), ctx.alloc(4 * max(1, n))
    bt = RxBatch(b.frames.ptr, b.frames_bytes, b.offset.ptr, b.length.ptr,
                 b.ptype.ptr if b.ptype is not None else None, n)
    _check(lib().udpdk_gpu_rss(ctx.handle, C.byref(bt), C.byref(RssOut(h.ptr, qo.ptr, qp.ptr))),
           "udpdk_gpu_rss")
    ctx.sync()
    out = (ctx.download(h, np.uint32, n), ctx.download(qo, np.uint32, cf.n_queues + 1),
           ctx.download(qp, np.uint32, n))
    for x in (h, qo, qp):
        x.free()
    return out


def download_ptr(ctx: GpuContext, ptr: int, dtype, count: int) -> np.ndarray:
    out = np.zeros(max(1, count), dtype)
    if count:
        _check(lib().udpdk_gpu_d2h(ctx.handle, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr),
                                   count * np.dtype(dtype).itemsize), "udpdk_gpu_d2h")
        ctx.sync()
    return out[:count]


def geometry(n: int, n_lanes: int) -> tuple[int, int]:
    t = C.c_uint32()
    k = C.c_uint32()
    _check(lib().udpdk_gpu_rx_geometry(n, n_lanes, C.byref(t), C.byref(k)), "rx_geometry")
    return t.value, k.value


# ---- host API helpers -----------------------------------------------------------------------------
SOL_SOCKET = socket.SOL_SOCKET
SO_REUSEADDR = socket.SO_REUSEADDR
SO_REUSEPORT = getattr(socket, "SO_REUSEPORT", 15)


def sockaddr_in(ip: str | int, port_host: int) -> bytes:
    """struct sockaddr_in with sin_port = htons(port_host)."""
    ipb = socket.inet_aton(ip) if isinstance(ip, str) else struct.pack("<I", ip)
    return struct.pack("<H", socket.AF_INET) + struct.pack(">H", port_host) + ipb + b"\0" * 8


def cmsg(level: int, typ: int, data: bytes) -> bytes:
    """One control message as CMSG_SPACE bytes (Linux, 64-bit: a 16-byte header, 8-byte alignment)."""
    ln = 16 + len(data)
    return (struct.pack("<QII", ln, level, typ) + data).ljust((ln + 7) & ~7, b"\0")


def raw_ip(ip: str) -> int:
    """Raw network-order IPv4 as the reference holds it (s_addr read as a LE integer)."""
    return struct.unpack("<I", socket.inet_aton(ip))[0]


def raw_port(port_host: int) -> int:
    return struct.unpack("<H", struct.pack(">H", port_host))[0]


class HostApi:
    """Thin wrappers around the udpdk_api.h calls (errno via ctypes.get_errno not used: the
    library sets the C errno; we read it through the libc symbol)."""

    def __init__(self):
        self.L = lib()
        self._errno = getattr(C.CDLL(None), "__errno_location")
        self._errno.restype = C.POINTER(C.c_int)

    def errno(self) -> int:
        return self._errno().contents.value

    def reset(self):
        self.L.udpdk_host_reset()

    def socket(self, domain=socket.AF_INET, typ=socket.SOCK_DGRAM, proto=0) -> int:
        return self.L.udpdk_socket(domain, typ, proto)

    def setsockopt(self, s, level, opt, val: int) -> int:
        v = C.c_int(val)
        return self.L.udpdk_setsockopt(s, level, opt, C.byref(v), 4)

    def getsockopt(self, s, level, opt) -> tuple[int, int]:
        v = C.c_int(-1)
        ln = C.c_uint32(4)
        rc = self.L.udpdk_getsockopt(s, level, opt, C.byref(v), C.byref(ln))
        return rc, v.value

    def bind(self, s, ip: str | int, port_host: int, addrlen: int = 16) -> int:
        a = C.create_string_buffer(sockaddr_in(ip, port_host), 16)
        return self.L.udpdk_bind(s, a, addrlen)

    def close(self, s) -> int:
        return self.L.udpdk_close(s)

    def sendto(self, s, payload: bytes, ip: str, port_host: int, flags: int = 0) -> int:
        a = C.create_string_buffer(sockaddr_in(ip, port_host), 16)
        buf = C.create_string_buffer(payload, max(1, len(payload)))
        return self.L.udpdk_sendto(s, buf, len(payload), flags, a, 16)

    def sendmsg(self, s, parts, ip=None, port_host: int = 0, *, gso: int | None = None, control: bytes | None = None,
                flags: int = 0) -> int:
        """udpdk_sendmsg: `parts` are the iovecs' bytes in order; ip None passes a NULL msg_name; gso adds
        a SOL_UDP / UDP_SEGMENT control message (control: raw control bytes instead)."""
        keep = [C.create_string_buffer(p, max(1, len(p))) for p in parts]
        iov = (IoVec * max(1, len(parts)))()
        for i, p in enumerate(parts):
            iov[i].iov_base = C.cast(keep[i], C.c_void_p)
            iov[i].iov_len = len(p)
        m = MsgHdr()
        if ip is not None:
            a = C.create_string_buffer(sockaddr_in(ip, port_host), 16)
            m.msg_name, m.msg_namelen = C.cast(a, C.c_void_p), 16
        m.msg_iov, m.msg_iovlen = iov, len(parts)
        if control is None and gso is not None:
            control = cmsg(SOL_UDP, UDP_SEGMENT, struct.pack("<H", gso))
        if control:
            cb = C.create_string_buffer(control, len(control))
            m.msg_control, m.msg_controllen = C.cast(cb, C.c_void_p), len(control)
        return self.L.udpdk_sendmsg(s, C.byref(m), flags)

    def gso_counts(self) -> dict[str, int]:
        c = GsoCounts()
        _check(self.L.udpdk_gso_counts(C.byref(c)), "udpdk_gso_counts")
        return {k: int(getattr(c, k)) for k, _ in GsoCounts._fields_}

    def recvfrom(self, s, maxlen: int = 2048):
        buf = C.create_string_buffer(maxlen)
        a = C.create_string_buffer(16)
        al = C.c_uint32(16)
        n = self.L.udpdk_recvfrom(s, buf, maxlen, 0, a, C.byref(al))
        if n < 0:
            return n, None, None
        port = struct.unpack(">H", a.raw[2:4])[0]
        ip = socket.inet_ntoa(a.raw[4:8])
        return n, buf.raw[:n], (ip, port)

    def connect(self, s, ip: str | int, port_host: int, addrlen: int = 16, family: int | None = None) -> int:
        """udpdk_connect; family=socket.AF_UNSPEC dissolves the association."""
        raw = sockaddr_in(ip, port_host)
        if family is not None:
            raw = struct.pack("<H", family) + raw[2:]
        a = C.create_string_buffer(raw, 16)
        return self.L.udpdk_connect(s, a, addrlen)

    def send(self, s, payload: bytes, flags: int = 0) -> int:
        buf = C.create_string_buffer(payload, max(1, len(payload)))
        return self.L.udpdk_send(s, buf, len(payload), flags)

    def sendto_null(self, s, payload: bytes, flags: int = 0) -> int:
        """udpdk_sendto with a NULL dest_addr (a connected socket's peer)."""
        buf = C.create_string_buffer(payload, max(1, len(payload)))
        return self.L.udpdk_sendto(s, buf, len(payload), flags, None, 0)

    def recv(self, s, maxlen: int = 2048):
        buf = C.create_string_buffer(maxlen)
        n = self.L.udpdk_recv(s, buf, maxlen, 0)
        return (n, None) if n < 0 else (n, buf.raw[:n])

    def _name(self, fn, s, addrlen: int):
        a = C.create_string_buffer(b"\xEE" * 16, 16)
        al = C.c_uint32(addrlen)
        rc = fn(s, a, C.byref(al))
        if rc != 0:
            return rc, None, al.value
        return rc, (socket.inet_ntoa(a.raw[4:8]), struct.unpack(">H", a.raw[2:4])[0]), al.value

    def getpeername(self, s, addrlen: int = 16):
        """(rc, (ip, port in host order) or None, the length written)."""
        return self._name(self.L.udpdk_getpeername, s, addrlen)

    def getsockname(self, s, addrlen: int = 16):
        return self._name(self.L.udpdk_getsockname, s, addrlen)

    def rx_refused(self) -> int:
        return int(self.L.udpdk_rx_refused())

    def peer_lanes(self, n: int) -> tuple[int, np.ndarray]:
        """udpdk_peer_lanes: (sockets connected, records[n] as PEER_DTYPE)."""
        t = np.zeros(max(1, n), PEER_DTYPE)
        t["ip"] = 0xEEEEEEEE
        rc = self.L.udpdk_peer_lanes(t.ctypes.data_as(C.c_void_p), n)
        return rc, t[:n]

    def tx_drain(self, max_frames=4096, cap=1 << 22):
        """Frames built on the GPU from the queued sends (needs udpdk_init)."""
        out = np.zeros(cap, np.uint8)
        off = np.zeros(max_frames, np.uint32)
        ln = np.zeros(max_frames, np.uint16)
        n = C.c_uint32()
        rc = self.L.udpdk_tx_drain(_ptr(out), cap, _ptr(off), _ptr(ln), max_frames, C.byref(n))
        if rc != 0:
            raise UdpdkError(f"udpdk_tx_drain errno={self.errno()}")
        return [bytes(out[off[i]:off[i] + ln[i]]) for i in range(n.value)]

    def tx_drain_raw(self, max_frames=4096, cap=1 << 22):
        """udpdk_tx_drain as it answers: (out[cap] pre-filled with 0xEE, out_off[n], out_len[n])."""
        out = np.full(cap, 0xEE, np.uint8)
        off = np.zeros(max(1, max_frames), np.uint32)
        ln = np.zeros(max(1, max_frames), np.uint16)
        n = C.c_uint32()
        rc = self.L.udpdk_tx_drain(_ptr(out), cap, _ptr(off), _ptr(ln), max_frames, C.byref(n))
        if rc != 0:
            raise UdpdkError(f"udpdk_tx_drain errno={self.errno()}")
        return out, off[:n.value].copy(), ln[:n.value].copy()

    def poll_echo(self, frames: np.ndarray, frames_bytes: int, offset: np.ndarray, length: np.ndarray,
                  ptype: np.ndarray | None = None, max_frames=4096, cap=1 << 22):
        """udpdk_poll_echo: (rc, errno, reply frames in order, RxStats, *n_out)."""
        offset = np.ascontiguousarray(offset, np.uint32)
        length = np.ascontiguousarray(length, np.uint16)
        pt = np.ascontiguousarray(ptype, np.uint32) if ptype is not None else None
        out = np.zeros(max(1, cap), np.uint8)
        off = np.zeros(max(1, max_frames), np.uint32)
        ln = np.zeros(max(1, max_frames), np.uint16)
        n = C.c_uint32(0xFFFFFFFF)
        st = RxStats()
        rc = self.L.udpdk_poll_echo(_ptr(frames), frames_bytes, _ptr(offset), _ptr(length),
                                    _ptr(pt) if pt is not None else None, len(offset), _ptr(out), cap,
                                    _ptr(off), _ptr(ln), max_frames, C.byref(n), C.byref(st))
        err = self.errno() if rc != 0 else 0
        return rc, err, [bytes(out[off[i]:off[i] + ln[i]]) for i in range(n.value if rc == 0 else 0)], st, n.value

    def config_icmp(self, flags: int) -> int:
        return lib().udpdk_config_icmp(int(flags))

    def config_icmp_burst(self, n: int) -> int:
        return lib().udpdk_config_icmp_burst(int(n))

    def icmp_counts(self) -> IcmpCounts:
        c = IcmpCounts()
        _check(lib().udpdk_icmp_counts(C.byref(c)), "udpdk_icmp_counts")
        return c

    def config_icmp_errors(self, on: int) -> int:
        """Received ICMP errors as pending socket errors (udpdk_config_icmp_errors): returns the previous
        setting; a negative `on` only reads it."""
        return self.L.udpdk_config_icmp_errors(int(on))

    def sock_error_post(self, s: int, ip: str | int, port_host: int, code: int) -> int:
        """udpdk_sock_error_post against the peer ip : port."""
        return self.L.udpdk_sock_error_post(s, raw_ip(ip) if isinstance(ip, str) else ip, raw_port(port_host), code)

    def rx_inject(self, s: int, payload: bytes, ip: str, port_host: int) -> int:
        """udpdk_sock_rx_inject; the bytes are kept alive by this object."""
        buf = C.create_string_buffer(payload, max(1, len(payload)))
        self._injected = getattr(self, "_injected", []) + [buf]
        return self.L.udpdk_sock_rx_inject(s, buf, len(payload), raw_ip(ip), raw_port(port_host))

    def icmp_err_counts(self) -> IcmpErrCounts:
        c = IcmpErrCounts()
        _check(self.L.udpdk_icmp_err_counts(C.byref(c)), "udpdk_icmp_err_counts")
        return c

    def config_arp(self, on: int) -> int:
        """ARP replies from udpdk_poll_rx (udpdk_config_arp): returns the previous setting; a negative
        `on` only reads it."""
        return self.L.udpdk_config_arp(int(on))

    def arp_announce(self) -> int:
        return self.L.udpdk_arp_announce()

    def config_mcast(self, on: int) -> int:
        """The membership filter and IGMP from udpdk_poll_rx (udpdk_config_mcast): returns the previous
        setting; a negative `on` only reads it."""
        return self.L.udpdk_config_mcast(int(on))

    def membership(self, s, opt: int, group: str | int, iface: str | int = 0, ifindex: int | None = None) -> int:
        """udpdk_setsockopt(s, IPPROTO_IP, opt, struct ip_mreq), or struct ip_mreqn when ifindex is given."""
        v = struct.pack("<II", raw_ip(group) if isinstance(group, str) else group,
                        raw_ip(iface) if isinstance(iface, str) else iface)
        if ifindex is not None:
            v += struct.pack("<i", ifindex)
        return self.L.udpdk_setsockopt(s, IPPROTO_IP, opt, C.create_string_buffer(v, len(v)), len(v))

    def join(self, s, group, iface=0) -> int:
        return self.membership(s, IP_ADD_MEMBERSHIP, group, iface)

    def leave(self, s, group, iface=0) -> int:
        return self.membership(s, IP_DROP_MEMBERSHIP, group, iface)

    def mcast_counts(self) -> dict:
        c = McastCounts()
        _check(self.L.udpdk_mcast_counts(C.byref(c)), "udpdk_mcast_counts")
        return {k: int(getattr(c, k)) for k, _ in McastCounts._fields_}

    def rx_not_member(self) -> int:
        return int(self.L.udpdk_rx_not_member())

    def arp_counts(self) -> ArpCounts:
        c = ArpCounts()
        _check(self.L.udpdk_arp_counts(C.byref(c)), "udpdk_arp_counts")
        return c

    def config_neigh(self, mode: int) -> int:
        """The neighbour cache (udpdk_config_neigh: 0 off, 1 strict, 2 fallback): returns the previous mode; a
        negative argument only reads it."""
        return self.L.udpdk_config_neigh(int(mode))

    def neigh_add(self, ip: str | int, mac: bytes) -> int:
        return self.L.udpdk_neigh_add(raw_ip(ip) if isinstance(ip, str) else ip, (C.c_uint8 * 6)(*mac))

    def neigh_flush(self) -> int:
        return self.L.udpdk_neigh_flush()

    def neigh_counts(self) -> dict[str, int]:
        c = NeighCounts()
        _check(self.L.udpdk_neigh_counts(C.byref(c)), "udpdk_neigh_counts")
        return {k: int(getattr(c, k)) for k, _ in NeighCounts._fields_}

    def tx_pending(self) -> int:
        return int(self.L.udpdk_tx_pending())

    def tx_dropped(self) -> int:
        return int(self.L.udpdk_tx_dropped())

    def rx_nobufs(self) -> int:
        return int(self.L.udpdk_rx_nobufs())

    def slots(self, n: int = 8):
        t = (Slot * n)()
        _check(self.L.udpdk_slot_table(t, n), "udpdk_slot_table")
        return [(t[i].ip, t[i].udp_port, t[i].bound) for i in range(n)]

    def config_set(self, src_mac: bytes, dst_mac: bytes, src_ip: str):
        s = C.create_string_buffer(src_mac, 6)
        d = C.create_string_buffer(dst_mac, 6)
        return self.L.udpdk_config_set(s, d, raw_ip(src_ip))

    def config_tx_cksum(self, on: int) -> int:
        """UDP checksum on sent datagrams (udpdk_config_tx_cksum): returns the previous setting;
        a negative `on` only reads it."""
        return self.L.udpdk_config_tx_cksum(int(on))

    def config_rx_drop(self, flags: int) -> int:
        """Deliveries udpdk_poll_rx drops for failed checksums or lengths (udpdk_config_rx_drop,
        RX_DROP_* flags): returns the previous flags; a negative argument only reads them."""
        return self.L.udpdk_config_rx_drop(int(flags))

    def rx_dropped(self) -> int:
        return int(self.L.udpdk_rx_dropped())

    def config_reuseport(self, mode: int) -> int:
        """How datagrams for several SO_REUSEPORT sockets are delivered (udpdk_config_reuseport,
        REUSEPORT_FANOUT / REUSEPORT_BALANCE): returns the previous mode; a negative argument only
        reads it."""
        return self.L.udpdk_config_reuseport(int(mode))

    def rx_balanced(self) -> int:
        return int(self.L.udpdk_rx_balanced())

    def reuseport_lanes(self, n: int) -> tuple[int, np.ndarray]:
        """udpdk_reuseport_lanes: (sockets flagged, flags[n])."""
        f = np.full(max(1, n), 0xEE, np.uint8)
        rc = self.L.udpdk_reuseport_lanes(f.ctypes.data_as(C.c_void_p), n)
        return rc, f[:n]

    def snapshot(self, compat: bool = False) -> BindSnapshot:
        snap = BindSnapshot()
        _check(self.L.udpdk_btable_snapshot(C.byref(snap), int(compat)), "udpdk_btable_snapshot")
        return snap

    def port_lists(self, compat: bool = False) -> dict[int, list[tuple[int, int, int]]]:
        s = self.snapshot(compat)
        out = {}
        for p in range(65536):
            c = s.port_count[p]
            if c:
                f = s.port_first[p]
                out[p] = [(s.binds[f + i].ip, s.binds[f + i].sockfd, s.binds[f + i].reuse) for i in range(c)]
        return out

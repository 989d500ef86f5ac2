/*
 * covt.h -- C-ABI of libcovt, the MI355X (gfx950) COVT Id/Geometry stream decoder.
 *
 * Drop-in boundary for the reference's Java decoder API (springmeyer/cov-tiles,
 * evaluation/java, package com.covt.decoder).  Each stream-level entry point
 * replaces one `public static` method of DecodingUtils.java with the same
 * argument order and meaning; the Java `IntWrapper pos` becomes an int32_t*
 * in/out cursor, `byte[]` inputs gain an explicit length, and outputs are
 * caller-provided arrays (the Java methods allocate theirs).  Decoding runs on
 * the GPU in every case: there is no CPU fallback.  A JNI shim
 * (cov-tiles_amd/jni/covt_jni.cc) binds these to
 * com.covt.decoder.gpu.GpuDecodingUtils; see INTEGRATION.md.
 *
 * Status codes map onto the Java exceptions of the reference:
 *   COVT_ERR_UNSUPPORTED_ENCODING -> IllegalArgumentException (CovtParser.java:426,443,460,475,493,508,571)
 *   COVT_ERR_TRUNCATED            -> ArrayIndexOutOfBoundsException / EOFException (ORC readers)
 *   COVT_ERR_COUNT_MISMATCH       -> ArrayIndexOutOfBoundsException (output overrun)
 *   COVT_ERR_BAD_HEADER           -> IllegalArgumentException (malformed FastPFOR / container)
 */
#ifndef COVT_H
#define COVT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COVT_OK 0
#define COVT_ERR_UNSUPPORTED_ENCODING (-1)
#define COVT_ERR_TRUNCATED (-2)
#define COVT_ERR_COUNT_MISMATCH (-3)
#define COVT_ERR_BAD_HEADER (-4)
#define COVT_ERR_DEVICE (-5)
#define COVT_ERR_INVALID_ARG (-6)

/* Device input buffers handed to the *_device entry points must start 16-byte aligned
 * and stay readable for COVT_INPUT_PADDING bytes past the last stream byte. */
#define COVT_INPUT_PADDING 4096

/* Container generations */
#define COVT_FORMAT_GENC 0 /* every committed fixture (test/fixtures/NAME/covt) */
#define COVT_FORMAT_GEND 1 /* what CovtParser.decodeCovt reads, CovtParser.java:574-652 */

/* Id column decode modes */
#define COVT_ID_FORMAT 0 /* format truth: VARINT = 64-bit LEB128, enc 4 = unsigned RLE */
#define COVT_ID_JAVA 1   /* CovtParser.decodedIds verbatim: 4-byte varint cap, enc 4 = zigzag-delta */

/* ---------------------------------------------------------------------------
 * Stream-level API: one function per DecodingUtils method.
 * `buf`/`buf_len` is the Java byte[]; *pos is the IntWrapper.  Host memory in and out.
 * ------------------------------------------------------------------------- */
/* DecodingUtils.decodeVarint(byte[] src, IntWrapper pos, int numValues)          DecodingUtils.java:35 */
int covt_decode_varint(const uint8_t* buf, size_t buf_len, int32_t* pos, int32_t num_values, int32_t* out);
/* DecodingUtils.decodeZigZagVarint(byte[], IntWrapper, int)                       DecodingUtils.java:46 */
int covt_decode_zigzag_varint(const uint8_t* buf, size_t buf_len, int32_t* pos, int32_t num_values, int32_t* out);
/* DecodingUtils.decodeZigZagDeltaVarint(byte[], IntWrapper, int)                  DecodingUtils.java:55 */
int covt_decode_zigzag_delta_varint(const uint8_t* buf, size_t buf_len, int32_t* pos, int32_t num_values,
                                    int32_t* out);
/* DecodingUtils.decodeZigZagDeltaVarintCoordinates(byte[], IntWrapper, int)       DecodingUtils.java:95 */
int covt_decode_zigzag_delta_varint_coordinates(const uint8_t* buf, size_t buf_len, int32_t* pos,
                                                int32_t num_values, int32_t* out);
/* DecodingUtils.decodeRle(byte[], int numValues, IntWrapper, boolean signed)      DecodingUtils.java:257
 * *pos advances by the bytes the RLE reader consumed; for ORC-writer-produced streams this equals
 * the Java advance (the length of the re-encoding, :268-270, :308-310). */
int covt_decode_rle(const uint8_t* buf, size_t buf_len, int32_t num_values, int32_t* pos, int32_t is_signed,
                    int64_t* out);
/* DecodingUtils.decodeByteRle(byte[], int numValues, IntWrapper, int byteLength)  DecodingUtils.java:275 */
int covt_decode_byte_rle(const uint8_t* buf, size_t buf_len, int32_t num_values, int32_t* pos, int32_t byte_length,
                         uint8_t* out);
/* DecodingUtils.decodeByteRle(byte[], int numValues, IntWrapper)                  DecodingUtils.java:290
 * (the form CovtParser.java:295 uses for Gen D present streams): *pos advances by the length of the
 * ORC RunLengthByteWriter re-encoding of the decoded values (getByteRleChunkSize :312-314). */
int covt_decode_byte_rle_reencode(const uint8_t* buf, size_t buf_len, int32_t num_values, int32_t* pos,
                                  uint8_t* out);
/* DecodingUtils.decodeFloatsLE(byte[], IntWrapper, int numValues)                 DecodingUtils.java:446
 * numValues little-endian floats copied out (host memory; no decode arithmetic). */
int covt_decode_floats_le(const uint8_t* buf, size_t buf_len, int32_t* pos, int32_t num_values, float* out);
/* DecodingUtils.decodeString(byte[], IntWrapper)                                  DecodingUtils.java:21
 * Reads the 4-byte-capped varint length and returns where the UTF-8 bytes lie (*str_off, *str_len);
 * *pos advances past them.  The JNI shim builds the java.lang.String from them. */
int covt_decode_string(const uint8_t* buf, size_t buf_len, int32_t* pos, int32_t* str_off, int32_t* str_len);
/* DecodingUtils.decodeFastPfor128ZigZagDelta(byte[], int, int byteLength, IntWrapper) DecodingUtils.java:316 */
int covt_decode_fastpfor_zigzag_delta(const uint8_t* buf, size_t buf_len, int32_t num_values, int32_t byte_length,
                                      int32_t* pos, int32_t* out);
/* DecodingUtils.decodeFastPfor128DeltaCoordinates(byte[], int, int, IntWrapper)   DecodingUtils.java:349 */
int covt_decode_fastpfor_delta_coordinates(const uint8_t* buf, size_t buf_len, int32_t num_values,
                                           int32_t byte_length, int32_t* pos, int32_t* out);
/* DecodingUtils.decodeDeltaVarintMortonCodes(byte[], IntWrapper, int numVertices, int numBits)
 *                                                                                 DecodingUtils.java:394
 * out holds 2*num_vertices ints (x,y interleaved). */
int covt_decode_delta_varint_morton_codes(const uint8_t* buf, size_t buf_len, int32_t* pos, int32_t num_vertices,
                                          int32_t num_bits, int32_t* out);
/* DecodingUtils.decodeFastPfor128DeltaMortonCodes(byte[], int, int, IntWrapper, int numBits)
 *                                                                                 DecodingUtils.java:411 */
int covt_decode_fastpfor_delta_morton_codes(const uint8_t* buf, size_t buf_len, int32_t num_vertices,
                                            int32_t byte_length, int32_t* pos, int32_t num_bits, int32_t* out);

/* ---------------------------------------------------------------------------
 * Batch API: the replacement for the per-tile CovtParser.decodeCovt loop
 * (CovtParser.java:53-133) restricted to the Id and Geometry columns.
 * ------------------------------------------------------------------------- */

/* Device-side decode operations (one per DecodingUtils codec x output type). */
enum covt_op {
    COVT_OP_NONE = 0,
    COVT_OP_BYTE_RLE_U8 = 1,            /* decodeByteRle -> uint8 (GeometryTypes, values <= 5 checked) */
    COVT_OP_RLE_U64 = 2,                /* decodeRle(signed=false) -> int64 (Id) */
    COVT_OP_RLE_I32 = 3,                /* decodeRle(signed=false) then (int) -> int32 (topology counts) */
    COVT_OP_RLE_S64 = 4,                /* decodeRle(signed=true) -> int64 */
    COVT_OP_VARINT_I32 = 5,             /* decodeVarint -> int32 */
    COVT_OP_VARINT_ZZ_I32 = 6,          /* decodeZigZagVarint -> int32 */
    COVT_OP_VARINT_ZZ_DELTA_I32 = 7,    /* decodeZigZagDeltaVarint -> int32 (VertexOffsets) */
    COVT_OP_VARINT_ZZ_DELTA_XY = 8,     /* decodeZigZagDeltaVarintCoordinates -> int32 x,y */
    COVT_OP_VARINT_DELTA_MORTON = 9,    /* decodeDeltaVarintMortonCodes -> int32 x,y per vertex */
    COVT_OP_FPF_ZZ_DELTA_I32 = 10,      /* decodeFastPfor128ZigZagDelta -> int32 */
    COVT_OP_FPF_ZZ_DELTA_XY = 11,       /* decodeFastPfor128DeltaCoordinates -> int32 x,y */
    COVT_OP_FPF_DELTA_MORTON = 12,      /* decodeFastPfor128DeltaMortonCodes -> int32 x,y per vertex */
    COVT_OP_VARINT_U64 = 13,            /* Id VARINT, format truth: 64-bit LEB128 -> int64 */
    COVT_OP_VARINT_I32_AS_I64 = 14,     /* Id VARINT, Java: decodeVarint then (long) */
    COVT_OP_VARINT_ZZ_DELTA_I64 = 15,   /* Id enc 4, Java: decodeZigZagDeltaVarint then (long) */
    COVT_OP_BYTE_RLE_RAW = 16,          /* decodeByteRle -> uint8, no value check (present / boolean bitsets) */
    COVT_OP_VARINT_ZZ_I32_AS_I64 = 17,  /* INT_64 VARINT_ZIG_ZAG, Java: decodeZigZagVarint then (long)
                                           (CovtParser.java:304-307) */
    COVT_OP_VARINT_ZZ_S64 = 18,         /* INT_64 VARINT_ZIG_ZAG, format truth: 64-bit LEB128, zigzag64 */
    COVT_OP_VARINT_ZZ_DELTA_S64 = 19,   /* INT_64 VARINT_DELTA_ZIG_ZAG, format truth: 64-bit, int64 running sum */
    COVT_OP_COUNT = 20
};

/* Codec families: each has its own kernel (register / LDS footprint), launched concurrently. */
#define COVT_FAMILY_RLE 0      /* byte RLE, integer RLE (and COVT_OP_NONE -> unsupported) */
#define COVT_FAMILY_VARINT 1   /* varint / zigzag / delta / Morton ops */
#define COVT_FAMILY_FASTPFOR 2 /* FastPFOR + VariableByte ops */
#define COVT_FAMILY_LANE 3     /* small RLE streams (flag COVT_DESC_LANE): one lane per stream */
#define COVT_FAMILY_SPLIT 4    /* long varint streams cut into chunks decoded by separate waves (COVT_DESC_SPLIT) */
#define COVT_FAMILY_SPLIT_FPF 5 /* long FastPFOR streams cut into chunks (COVT_DESC_SPLIT | COVT_DESC_SPLIT_FPF) */
#define COVT_FAMILY_SPLIT_RLE 6 /* long ORC RLE streams cut at group starts (COVT_DESC_SPLIT | COVT_DESC_SPLIT_RLE) */
#define COVT_NUM_FAMILIES 7

/* covt_stream_desc.flags */
#define COVT_DESC_LANE 0x1u /* decoded by the lane-per-stream kernel (set by the plan for small streams) */
/* Long streams (plan rule: varint ops -- Java-capped and 64-bit LEB128 -- and FastPFOR ops whose cost, bytes
 * + output bytes / 4, exceeds COVT_SPLIT_MIN and the plan's total / COVT_SPLIT_RATIO) are
 * cut into chunks of COVT_SPLIT_CHUNK bytes (varint) or COVT_SPLIT_VALUES values (FastPFOR, whole
 * blocks), each decoded by its own wave; a chunk's value index and running
 * sums come from its predecessors by a decoupled look-back.  A chunk is COVT_SPLIT_SLOTS consecutive
 * descriptors: the chunk descriptor (flags COVT_DESC_SPLIT, avail = chunk index, the other fields those
 * of the stream) and pads (COVT_DESC_SPLIT_PAD; the first carries the chunk's range [in_off, out_off):
 * stream-relative bytes, or values for FastPFOR), whose result entries hold the look-back records.  The stream's result is
 * written to its chunk 0's entry.  Split descriptors need the grouped launch. */
#define COVT_DESC_SPLIT 0x2u
#define COVT_DESC_SPLIT_PAD 0x4u
#define COVT_DESC_SPLIT_FPF 0x8u /* with SPLIT / SPLIT_PAD: a FastPFOR stream's chunk (pads [2..7]: the plan's
                                  * walk of the headers before it -- int32 slots in every field but
                                  * op / num_bits / flags; all zero = none, the chunk walks them itself) */
#define COVT_DESC_SPLIT_RLE 0x10u /* with SPLIT / SPLIT_PAD: an ORC RLE stream's chunk (whole groups, located by the
                                   * plan; pads [1] bytes [s, e), [2] values (first, count), [3] consumed) */
#define COVT_SPLIT_SLOTS 8
#define COVT_SPLIT_CHUNK 2048 /* default varint / RLE chunk bytes (covt_plan_options.split_chunk) */
#define COVT_SPLIT_VALUES 2048 /* default FastPFOR chunk values, whole blocks (covt_plan_options.split_values) */
#define COVT_SPLIT_MIN 8192   /* default: streams costlier than this are split (covt_plan_options.split_min) */
#define COVT_SPLIT_RATIO 3000 /* ... and than the plan's total cost / this (covt_plan_options.split_ratio) */
#define COVT_LANE_MAX_BYTES 128     /* covt_plan_options.lane_max_bytes 0 (auto): Id / Geometry plans */
#define COVT_LANE_MAX_BYTES_PROPS 512 /* ... plans with COVT_PLAN_PROPERTIES */
#define COVT_LANE_MAX_VALUES 256    /* covt_plan_options.lane_max_values 0 (auto): Id / Geometry plans */
#define COVT_LANE_MAX_VALUES_PROPS 512 /* ... plans with COVT_PLAN_PROPERTIES */
#define COVT_LANE_MIN_STREAMS 65536 /* default covt_plan_options.lane_min_streams */
#define COVT_SPLIT_MAX_STREAMS 65536 /* default covt_plan_options.split_max_streams */

/* Plan-layout options.  Every plan property that used to be steered by the environment is a field
 * here: a library inside a JVM or tile server plans the same way whatever its process inherited.
 * Initialise with covt_plan_options_init (the defaults below), change fields, pass to
 * covt_plan_create_opts / covt_device_plan_create_opts.  Plans made with equal options from equal
 * tiles are byte-identical, host or device. */
typedef struct covt_plan_options {
    uint32_t size;             /* sizeof(covt_plan_options), set by covt_plan_options_init */
    uint32_t flags;            /* COVT_PLAN_PROPERTIES (host plans only) */
    int64_t split_min;         /* split streams whose cost (bytes + output bytes / 4) exceeds this and ... */
    int64_t split_ratio;       /* ... the plan's total cost / split_ratio (0: no batch-relative bound);
                                  split_min < 0: never split */
    int64_t split_chunk;       /* bytes of cost per varint / RLE chunk (>= 64) */
    int64_t split_values;      /* values per FastPFOR chunk (a multiple of 256, >= 256) */
    int32_t fpf_split_weight;  /* a FastPFOR stream's output counted this many times in its split cost (>= 1) */
    int32_t lane_max_bytes;    /* RLE streams of <= this many bytes (<= 65535; 0: auto, COVT_LANE_MAX_BYTES or
                                  _PROPS with property columns) and <= lane_max_values values go to the lane family ... */
    int64_t lane_min_streams;  /* ... when the plan holds at least this many of them (lane_max_bytes < 0: never) */
    int32_t plan_threads;      /* host threads of covt_plan_create (0: min(hardware threads, 16)) */
    int32_t host_prefault;     /* decode_host into pageable memory: fault the output pages in on host threads
                                  while the device works (1, default) or not (0) */
    int32_t prefault_threads;  /* those threads (default 8) */
    int32_t device_walk;       /* covt_device_plan: 0 = a wave per tile with per-tile slots (default),
                                  1 = the same walk twice (no slots), k >= 2: k tiles per workgroup, a lane each */
    int32_t lane_max_values;   /* the lane family's value limit (<= 32767; 0: auto, COVT_LANE_MAX_VALUES or _PROPS with
                                  property columns, whose many small dictionary-index streams favour longer lanes) */
    int64_t split_max_streams; /* plans of more streams than this split nothing (0: no bound).  Enough streams keep
                                  every wave slot busy, and there the chunks' header re-walks and look-back cost
                                  more than the long poles they shorten */
    int32_t split_grow;        /* 1 (default): split_chunk / split_values doubled for plans of >= 4 MiB of cost and
                                  quadrupled from 48 MiB (covt_split_plan.h split_grow_factor); 0: fixed */
} covt_plan_options;
void covt_plan_options_init(covt_plan_options* opts);

/* One device-resident plan entry (32 bytes). */
typedef struct covt_stream_desc {
    uint64_t in_off;     /* payload byte offset in the batch input buffer */
    uint64_t out_off;    /* output byte offset in the batch output buffer (plans: 128-byte aligned) */
    int32_t avail;       /* readable payload bytes (byteLength for plans; buf_len-pos for stream calls) */
    int32_t num_values;  /* values (vertices for the Morton ops) to produce */
    uint8_t op;          /* enum covt_op */
    uint8_t num_bits;    /* Morton bits, 32 - nlz(extent) (CovtParser.java:77) */
    uint16_t flags;      /* COVT_DESC_* */
    int32_t byte_length; /* wire byteLength (FastPFOR reads byteLength/4 big-endian words) */
} covt_stream_desc;

/* Per-stream result written by the kernel.  consumed is 0 whenever status != COVT_OK, on every decode path
 * (wave-per-stream, lane-per-stream, split chunks): a failed stream's row does not depend on which kernel the
 * plan gave it to, so a batch and its shards report the same rows. */
typedef struct covt_stream_result {
    int32_t status;   /* COVT_OK or a negative COVT_ERR_* */
    int32_t consumed; /* payload bytes consumed (FastPFOR / byte RLE: byteLength); 0 unless status is COVT_OK */
} covt_stream_result;

/* Host-visible stream record of a plan, in tile order. */
typedef struct covt_stream_info {
    int32_t tile, layer, column_kind, stream_type; /* column_kind: 0 id, 1 geometry */
    int32_t encoding, column_type, num_values, byte_length;
    int32_t num_bits, op, elem_bytes, desc_index; /* desc_index: row in the launch-ordered descs */
    int64_t in_off, out_off, out_elems;
} covt_stream_info;

typedef struct covt_plan covt_plan;

/* Walk the container metadata of n_tiles tiles held back to back in `bytes` (host memory) and
 * build the descriptor table.  Tiles that fail to walk get a negative tile status and no streams. */
int covt_plan_create(const uint8_t* bytes, const uint64_t* tile_offsets, const uint64_t* tile_sizes,
                     int32_t n_tiles, int32_t format, int32_t id_mode, covt_plan** out);
void covt_plan_destroy(covt_plan* plan);
int64_t covt_plan_num_streams(const covt_plan* plan);
int64_t covt_plan_output_bytes(const covt_plan* plan);
/* stream-byte, output-byte and vertex totals over all planned streams */
int covt_plan_totals(const covt_plan* plan, int64_t* in_bytes, int64_t* out_bytes, int64_t* vertices);
int covt_plan_streams(const covt_plan* plan, covt_stream_info* out);    /* num_streams records */
int64_t covt_plan_num_descs(const covt_plan* plan);  /* descriptors (>= streams: split chunks and pads) */
int covt_plan_descs(const covt_plan* plan, covt_stream_desc* out);      /* num_descs, launch order */
/* plan-order stream index of every descriptor (launch order); a stream's result is at its
 * covt_stream_info.desc_index */
int covt_plan_desc_streams(const covt_plan* plan, int64_t* out);
/* Launch order groups descriptors by family (RLE, varint, FastPFOR, lane; largest stream first inside
 * a family, the lane family also by op): counts[f] = descriptors of family f. */
int covt_plan_family_counts(const covt_plan* plan, int64_t counts[COVT_NUM_FAMILIES]);
int covt_plan_tile_status(const covt_plan* plan, int32_t* out);         /* n_tiles */

/* Launch the decode of n_streams descriptors on `hip_stream` (a hipStream_t; NULL = default).
 * d_in: batch bytes on the device (see COVT_INPUT_PADDING); d_desc: descriptors on the device;
 * d_out: output buffer of covt_plan_output_bytes bytes; d_res: n_streams results.  Asynchronous.
 * Split descriptors (COVT_DESC_SPLIT / _PAD) are skipped here: they need the grouped launch. */
int covt_decode_streams_device(const uint8_t* d_in, const covt_stream_desc* d_desc, int64_t n_streams,
                               uint8_t* d_out, covt_stream_result* d_res, void* hip_stream);

/* Same, for descriptors grouped by family (as covt_plan_descs returns them): the family kernels run
 * concurrently on forked streams joined back into `hip_stream`.  d_res holds one entry per
 * descriptor (covt_plan_num_descs); results are at the streams' desc_index entries. */
int covt_decode_streams_device_grouped(const uint8_t* d_in, const covt_stream_desc* d_desc,
                                       const int64_t family_counts[COVT_NUM_FAMILIES], uint8_t* d_out,
                                       covt_stream_result* d_res, void* hip_stream);
/* The same launch with its shape chosen by the caller: COVT_LAUNCH_AUTO (what the call above does: one
 * fused kernel for batches of at most 4096 waves, else the per-family kernels on forked streams),
 * COVT_LAUNCH_FUSED or COVT_LAUNCH_FORKED whatever the batch size (tests pin both code paths; outputs
 * and results are identical). */
#define COVT_LAUNCH_AUTO 0
#define COVT_LAUNCH_FUSED 1
#define COVT_LAUNCH_FORKED 2
/* or-ed into launch_mode: the FastPFOR family's kernel variant in a forked launch.  By default (neither) a
 * family of at least 65,536 streams takes the streamed variant (packed words through an LDS ring, block
 * headers 64 at a time, a batch's exception words gathered at once: the shorter launch for large batches) and
 * smaller ones the per-block pipeline (shorter for strong-scaling shards); both give identical results. */
#define COVT_LAUNCH_FPF_STREAM 0x4
#define COVT_LAUNCH_FPF_CLASSIC 0x8
int covt_decode_streams_device_grouped_mode(const uint8_t* d_in, const covt_stream_desc* d_desc,
                                            const int64_t family_counts[COVT_NUM_FAMILIES], uint8_t* d_out,
                                            covt_stream_result* d_res, void* hip_stream, int32_t launch_mode);

/* Host entry point: H2D + decode + D2H for host tiles on the current device.
 * bytes/n_bytes: the caller's buffer the plan's tile offsets index (every tile must lie inside
 * [0, n_bytes), else COVT_ERR_INVALID_ARG); host_out: covt_plan_output_bytes(plan) bytes, stream i's
 * values at covt_stream_info.out_off; host_res: num_streams results (plan stream order).  Bytes of
 * host_out outside the stream slices (16-byte alignment padding) are unspecified.
 * Device buffers and the descriptor table stay cached on the plan across calls (released by
 * covt_plan_release_device or covt_plan_destroy); calls on one plan are serialised. */
int covt_plan_decode_host(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, uint8_t* host_out,
                          covt_stream_result* host_res);

/* Multi-GPU host entry point: shards the plan's tiles over min(n_gpus, devices) devices (contiguous
 * tile ranges balanced on stream + output bytes, one host thread per device, no collectives); each
 * shard is one H2D, one launch and one D2H into its part of host_out.  Same results as
 * covt_plan_decode_host. */
int covt_plan_decode_host_multi(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, int32_t n_gpus,
                                uint8_t* host_out, covt_stream_result* host_res);

/* The same with an explicit shard -> device map: n_shards shards, shard k on device shard_devices[k]
 * (devices may repeat: several shards of one device run concurrently on their own streams). */
int covt_plan_decode_host_shards(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, int32_t n_shards,
                                 const int32_t* shard_devices, uint8_t* host_out, covt_stream_result* host_res);

/* Free the device buffers the host entry points cached on this plan. */
int covt_plan_release_device(const covt_plan* plan);

/* ---------------------------------------------------------------------------
 * Geometry assembly: the GPU replacement for
 * CovtParser.convertGeometryColumn (CovtParser.java:135-274, getLineString / getLinearRing /
 * getICELineString :513-550).  Java builds one JTS Geometry per feature out of the decoded
 * GeometryColumn; here every geometry column of a plan becomes one GeoArrow-style nested-offset
 * record, computed on the device from the decoded streams (prefix sums of the count streams,
 * ICE vertex gather):
 *
 *   geometry_offsets[n_features + 1]  feature -> parts    (POINT/LINESTRING/POLYGON: 1 part,
 *                                                          MULTI*: geometryOffsets count)
 *   part_offsets[num_parts + 1]       part -> rings       (POLYGON parts: partOffsets count,
 *                                                          point / line parts: 1 ring)
 *   ring_offsets[num_rings + 1]       ring -> coordinates (point: 1, line: partOffsets count,
 *                                                          polygon ring: ringOffsets count, closed)
 *   coords[2 * num_coords]            int32 x,y (ICE: vertexBuffer[2*vertexOffsets[i]], +0/+1)
 *
 * Offsets are absolute within the column and start at 0; types[] of the decoded GeometryTypes
 * stream says how to read a feature.  Polygon rings are closed as JTS LinearRings are
 * (getLinearRing appends the first vertex): a ring whose stream omits the closing vertex gets it
 * appended; Gen C ICE rings already carry it and are copied as they are.
 * Deviations from the Java method, decided for format truth: the MULTIPOLYGON bugs of SURVEY Q7
 * (CovtParser.java:237-259) are not reproduced, and MULTIPOINT (which Java rejects with
 * IllegalArgumentException) reads one geometryOffsets count of points.
 * ------------------------------------------------------------------------- */
#define COVT_GEOM_CLOSED_IN_STREAM 0x1u /* polygon rings carry their closing vertex in the stream */
#define COVT_GEOM_TOO_LARGE 0x80000000u /* over COVT_GEOM_MAX_CAP: not assembled (COVT_ERR_INVALID_ARG) */

/* One device-resident geometry-column entry (160 bytes). */
typedef struct covt_geom_desc {
    int64_t in_off[6];   /* decode-output byte offsets of the GeometryTypes, GeometryOffsets, PartOffsets,
                            RingOffsets, VertexOffsets, VertexBuffer arrays (-1: stream absent) */
    int32_t in_len[6];   /* their element counts (VertexBuffer: vertices) */
    int32_t in_res[6];   /* their row in the decode result array (-1: absent) */
    int64_t out_off[6];  /* assembly-output byte offsets: geometry_offsets, part_offsets, ring_offsets,
                            coords, part scratch, ring scratch (16-byte aligned) */
    int32_t part_cap, ring_cap, coord_cap; /* capacities the output slices were sized for */
    int32_t flags;                         /* COVT_GEOM_* */
} covt_geom_desc;

/* Per-column assembly result written by the kernel. */
typedef struct covt_geom_result {
    int32_t status; /* COVT_OK, a source stream's decode status, or a COVT_ERR_* of the assembly */
    int32_t num_parts, num_rings, num_coords;
} covt_geom_result;

/* Host-visible geometry-column record of a plan, in tile order. */
typedef struct covt_geom_info {
    int32_t tile, layer, column_type, n_features;
    int32_t stream[6]; /* tile-order stream index of each source stream (-1: absent) */
    int32_t part_cap, ring_cap, coord_cap, flags;
    int32_t desc_index, reserved; /* desc_index: row in the launch-ordered geometry descriptors */
    int64_t out_off[6];
} covt_geom_info;

/* Column capacities are bounded so the kernel's 32-bit scans cannot wrap; a larger column
 * (over 2^25 rings or coordinates) is flagged COVT_GEOM_TOO_LARGE and not assembled. */
#define COVT_GEOM_MAX_CAP (1 << 25)

int64_t covt_plan_num_geometry_columns(const covt_plan* plan);
int64_t covt_plan_assembly_bytes(const covt_plan* plan); /* size of the assembly output buffer */
int covt_plan_geometry_columns(const covt_plan* plan, covt_geom_info* out); /* tile order */
int covt_plan_geometry_descs(const covt_plan* plan, covt_geom_desc* out);   /* launch order (largest first) */

/* Assemble every geometry column on `hip_stream` after the decode launch of the same plan:
 * d_decoded / d_res are the decode output and result arrays (launch-order results), d_gdesc the
 * geometry descriptors, d_asm an output buffer of covt_plan_assembly_bytes bytes, d_gres
 * n_columns results (in d_gdesc order).  Asynchronous. */
int covt_assemble_geometry_device(const uint8_t* d_decoded, const covt_stream_result* d_res,
                                  const covt_geom_desc* d_gdesc, int64_t n_columns, uint8_t* d_asm,
                                  covt_geom_result* d_gres, void* hip_stream);

/* Convenience: H2D + decode + assembly + D2H of the whole plan on the current device.
 * host_asm: covt_plan_assembly_bytes bytes; host_gres: one result per column in tile order. */
int covt_plan_assemble_host(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, uint8_t* host_asm,
                            covt_geom_result* host_gres);

/* ---------------------------------------------------------------------------
 * Geometry as WKB: the last step of CovtParser.convertGeometryColumn (CovtParser.java:135-274), whose
 * result is one JTS Geometry per feature.  Every assembled geometry column of a plan becomes one Arrow
 * `binary` column holding one little-endian ISO WKB value per feature, which JTS (WKBReader), GeoParquet,
 * PostGIS, GDAL and shapely read as it is:
 *
 *   wkb_offsets[n_features + 1]  int32 byte offsets into the column's own byte slice (first 0, last =
 *                                the column's byte count, covt_wkb_result.n_bytes)
 *   wkb_bytes                    the features' WKB values back to back, in feature order
 *
 * Byte order 1 (NDR), geometry code = GeometryTypes ordinal + 1 (POINT 1 ... MULTIPOLYGON 6), 2-D, no
 * SRID; counts uint32, coordinates float64 of the assembled int32 x, y (exact).  The structure is the
 * assembled column's, format truth as above: polygon rings closed as assembly left them, empty parts and
 * rings written with count 0, a degenerate ring JTS would reject written as the stream has it.
 * With G parts, R rings and C coordinates in a feature its value takes
 *   POINT 21, LINESTRING 9 + 16 C, POLYGON 9 + 4 R + 16 C, MULTIPOINT 9 + 21 G,
 *   MULTILINESTRING 9 + 9 G + 16 C, MULTIPOLYGON 9 + 9 G + 4 R + 16 C  bytes,
 * so a column's slice of 9 (n_features + part_cap) + 4 ring_cap + 16 coord_cap bytes always suffices.
 * The pass runs after covt_assemble_geometry_device on the same stream: a scan of the per-feature sizes,
 * then every coordinate, ring count, part header and feature header stored at its closed-form address.
 * Statuses: a column whose assembly result is not COVT_OK gets that status (n_bytes 0, slices untouched);
 * COVT_GEOM_TOO_LARGE, COVT_WKB_TOO_LARGE or a byte_cap over INT32_MAX -> COVT_ERR_INVALID_ARG; a byte
 * total over byte_cap -> COVT_ERR_COUNT_MISMATCH (no byte of the byte slice written).
 * ------------------------------------------------------------------------- */
#define COVT_WKB_TOO_LARGE 0x1 /* covt_wkb_desc.flags: the column's capacity does not fit int32 offsets */

/* One device-resident WKB column entry (32 bytes), parallel to covt_geom_desc (launch order). */
typedef struct covt_wkb_desc {
    int64_t offsets_off; /* byte offset of wkb_offsets in the WKB output buffer (16-byte aligned) */
    int64_t bytes_off;   /* byte offset of wkb_bytes (16-byte aligned) */
    int64_t byte_cap;    /* bytes the wkb_bytes slice holds */
    int32_t n_features, flags;
} covt_wkb_desc;

/* Per-column WKB result written by the kernel. */
typedef struct covt_wkb_result {
    int32_t status, reserved;
    int64_t n_bytes; /* bytes of WKB written (0 unless status is COVT_OK) */
} covt_wkb_result;

/* Host-visible WKB column record of a plan, in tile order (48 bytes); column c belongs to geometry
 * column c (covt_geom_info). */
typedef struct covt_wkb_info {
    int32_t tile, layer, n_features, desc_index; /* desc_index: row in the launch-ordered descriptors */
    int64_t offsets_off, bytes_off, byte_cap;
    int32_t flags, reserved;
} covt_wkb_info;

int64_t covt_plan_wkb_bytes(const covt_plan* plan); /* size of the WKB output buffer */
int covt_plan_wkb_columns(const covt_plan* plan, covt_wkb_info* out); /* tile order, num_geometry_columns */
int covt_plan_wkb_descs(const covt_plan* plan, covt_wkb_desc* out);   /* launch order (= covt_plan_geometry_descs) */

/* Serialize every assembled geometry column on `hip_stream`, after covt_assemble_geometry_device on the
 * same stream: d_decoded the decode output (GeometryTypes are read from it at covt_geom_desc.in_off[0]),
 * d_gdesc / d_asm / d_gres the assembly's descriptors, output and results, d_wdesc the WKB descriptors
 * (same order), d_wkb an output buffer of covt_plan_wkb_bytes bytes, d_wres n_columns results (same
 * order).  Asynchronous; needs no scratch, so it can be captured in a HIP graph as it is. */
int covt_geometry_wkb_device(const uint8_t* d_decoded, const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                             const covt_geom_result* d_gres, const covt_wkb_desc* d_wdesc, int64_t n_columns,
                             uint8_t* d_wkb, covt_wkb_result* d_wres, void* hip_stream);

/* Convenience: H2D + decode + assembly + WKB + D2H of the whole plan on the current device.
 * host_wkb: covt_plan_wkb_bytes bytes; host_wres: one result per column in tile order. */
int covt_plan_wkb_host(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, uint8_t* host_wkb,
                       covt_wkb_result* host_wres);

/* ---------------------------------------------------------------------------
 * Geometry bounding boxes: the GeoParquet 1.1 bbox covering column of every assembled geometry column,
 * the companion of its WKB column.  Per column one slice of 32 * n_features bytes (16-byte aligned start):
 *
 *   xmin[n_features] | ymin[n_features] | xmax[n_features] | ymax[n_features]     float64, back to back
 *
 * the struct-of-arrays layout of an Arrow struct<xmin, ymin, xmax, ymax: double>.  A value is the min / max
 * of the feature's assembled int32 x or y as float64 (exact), over every coordinate the assembled column
 * attributes to the feature: coords[ring_offsets[part_offsets[geometry_offsets[f]]] ..
 * ring_offsets[part_offsets[geometry_offsets[f + 1]]]), the ring-closing vertex included, whatever the
 * geometry type.  A feature with no coordinate (a MULTI* of 0 parts, a line of 0 vertices, a polygon whose
 * rings are all empty) gets the quiet NaN 0x7FF8000000000000 in all four arrays, as shapely.bounds reports
 * an empty geometry.  Coordinates are tile-local, the space of coords and of the WKB values (both in a CRS:
 * "Georeferenced geometry" below).
 * Per column a covt_bbox_result: extent = xmin, ymin, xmax, ymax over all the column's coordinates (the
 * layer's bbox in GeoParquet file metadata, row-group statistics; all NaN without a coordinate), n_empty
 * the number of NaN rows.
 * Statuses: a column whose assembly result is not COVT_OK gets that status (n_empty 0, extent NaN, slice
 * untouched); COVT_GEOM_TOO_LARGE or COVT_BBOX_TOO_LARGE -> COVT_ERR_INVALID_ARG, likewise.
 * ------------------------------------------------------------------------- */
#define COVT_BBOX_TOO_LARGE 0x1 /* covt_bbox_desc.flags: assembly refuses the column (COVT_GEOM_TOO_LARGE) */

/* One device-resident bounding-box column entry (16 bytes), parallel to covt_geom_desc (launch order). */
typedef struct covt_bbox_desc {
    int64_t off; /* byte offset of the column's slice in the bounding-box output buffer (16-byte aligned) */
    int32_t n_features, flags;
} covt_bbox_desc;

/* Per-column bounding-box result written by the kernels (40 bytes). */
typedef struct covt_bbox_result {
    int32_t status, n_empty;
    double extent[4]; /* xmin, ymin, xmax, ymax of the column (NaN: no coordinate, or status not COVT_OK) */
} covt_bbox_result;

/* Host-visible bounding-box column record of a plan, in tile order (32 bytes); column c belongs to
 * geometry column c (covt_geom_info). */
typedef struct covt_bbox_info {
    int32_t tile, layer, n_features, desc_index; /* desc_index: row in the launch-ordered descriptors */
    int64_t off;
    int32_t flags, reserved;
} covt_bbox_info;

int64_t covt_plan_bbox_bytes(const covt_plan* plan); /* size of the bounding-box output buffer */
int covt_plan_bbox_columns(const covt_plan* plan, covt_bbox_info* out); /* tile order, num_geometry_columns */
int covt_plan_bbox_descs(const covt_plan* plan, covt_bbox_desc* out);   /* launch order (= covt_plan_geometry_descs) */

/* Bounding boxes of every assembled geometry column on `hip_stream`, after covt_assemble_geometry_device
 * on the same stream: d_gdesc / d_asm / d_gres the assembly's descriptors, output and results, d_bdesc the
 * bounding-box descriptors (same order), d_bbox an output buffer of covt_plan_bbox_bytes bytes, d_bres
 * n_columns results (same order).  Asynchronous; needs no scratch and writes every output double exactly
 * once, so it can be captured in a HIP graph as it is and its result does not depend on scheduling. */
int covt_geometry_bbox_device(const covt_geom_desc* d_gdesc, const uint8_t* d_asm, const covt_geom_result* d_gres,
                              const covt_bbox_desc* d_bdesc, int64_t n_columns, uint8_t* d_bbox,
                              covt_bbox_result* d_bres, void* hip_stream);

/* Convenience: H2D + decode + assembly + bounding boxes + D2H of the whole plan on the current device.
 * host_bbox: covt_plan_bbox_bytes bytes; host_bres: one result per column in tile order. */
int covt_plan_bbox_host(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, uint8_t* host_bbox,
                        covt_bbox_result* host_bres);

/* ---------------------------------------------------------------------------
 * Geometry measures: how big every feature of an assembled geometry column is, what JTS answers with
 * Geometry.getArea(), getLength() and getNumPoints() and a tile server, a GeoParquet writer or a simplifier
 * asks next (drop small features per zoom, store area / length beside bbox, size work by vertex count).
 * Per column one slice (16-byte aligned start) in the measures output buffer:
 *
 *   area[n_features] float64 | length[n_features] float64 | num_coords[n_features] int32 (padded to 16 bytes)
 *   | per-ring scratch, 16 * ring_cap bytes (contents unspecified)
 *
 * The scratch (a ring's doubled signed area and its length) lives in the same buffer, sized by the same
 * layout rule from the column's ring_cap, so the pass allocates nothing.  All values are in tile pixels and
 * are taken over the assembled column as the bounding boxes are: the ring-closing vertex is included and no
 * implicit closing edge is added.  With ring r's coordinates (x_0, y_0) .. (x_{m-1}, y_{m-1}),
 * m = ring_offsets[r + 1] - ring_offsets[r], and t the feature's GeometryTypes ordinal:
 *
 *   num_coords[f] = start(f + 1) - start(f), start(f) = ring_offsets[part_offsets[geometry_offsets[f]]]: the
 *     number of points in the feature's WKB value.
 *   area[f]: every ring has S_r = sum over i in 0 .. m - 2 of (x_i * y_{i+1} - x_{i+1} * y_i) in int64 (a
 *     product of two int32 is exact; differences and sums are two's complement mod 2^64; 0 for m < 2).  For
 *     POLYGON (2) and MULTIPOLYGON (5), T_f = sum over the parts p of f of (|S of p's first ring| - sum of |S_r|
 *     over p's other rings), |.| the magnitude as uint64, the sum mod 2^64 and then read as int64, and
 *     area[f] = (double)T_f * 0.5.  Every other type gets +0.0.  This is JTS Polygon.getArea: shell minus
 *     holes, each by absolute value, whatever the winding.  Integer arithmetic, so the value does not depend
 *     on evaluation order.  It is the true area whenever the sum of the |terms| is below 2^63 and
 *     |T_f| < 2^54, which every real tile meets (coordinates lie within a few extents of 4096); outside that
 *     bound the mod-2^64 arithmetic as written is the definition (a hole larger than its shell gives a
 *     negative area).
 *   length[f]: for types 1, 2, 4 and 5 (lines, and polygon perimeters as JTS getLength) the sum over all the
 *     feature's rings and all i in 0 .. m - 2 of sqrt(dx * dx + dy * dy), dx and dy the exact coordinate
 *     differences as float64 (a difference of two int32 is exact), one rounding per operation and no fused
 *     multiply-add.  POINT and MULTIPOINT get +0.0.  The summation order is the kernel's; the value is within
 *     (m_f + 4) * 2^-52 relative of the exactly rounded sum, m_f the feature's segment count: a few roundings
 *     per term, well inside 2^-51, and at most m_f - 1 roundings in a sum of non-negative terms in any order.
 *     No floating-point atomics are used, so the same input through the same entry point gives the same bytes
 *     every time.
 *
 * A feature without coordinates gets 0.0, 0.0, 0.  Per column a covt_measures_result.
 * Statuses: a column whose assembly result is not COVT_OK gets that status (slice untouched);
 * COVT_GEOM_TOO_LARGE or COVT_MEASURES_TOO_LARGE -> COVT_ERR_INVALID_ARG, likewise.
 * Out of scope: measures in a CRS (for Web Mercator multiply length by |sx| and area by sx * sx of the
 * column's covt_geo_xform; degrees have no meaningful area), centroids, per-column totals.
 * ------------------------------------------------------------------------- */
#define COVT_MEASURES_TOO_LARGE 0x1 /* covt_measures_desc.flags: assembly refuses the column (COVT_GEOM_TOO_LARGE) */

/* One device-resident measures column entry (24 bytes), parallel to covt_geom_desc (launch order). */
typedef struct covt_measures_desc {
    int64_t off; /* byte offset of the column's slice in the measures output buffer (16-byte aligned) */
    int32_t n_features, flags;
    int32_t ring_cap, reserved; /* ring_cap: the rings the slice's scratch holds (= covt_geom_desc.ring_cap) */
} covt_measures_desc;

/* Per-column measures result written by the kernels (8 bytes). */
typedef struct covt_measures_result {
    int32_t status, reserved;
} covt_measures_result;

/* Host-visible measures column record of a plan, in tile order (32 bytes); column c belongs to geometry
 * column c (covt_geom_info). */
typedef struct covt_measures_info {
    int32_t tile, layer, n_features, desc_index; /* desc_index: row in the launch-ordered descriptors */
    int64_t off;
    int32_t flags, ring_cap;
} covt_measures_info;

int64_t covt_plan_measures_bytes(const covt_plan* plan); /* size of the measures output buffer */
int covt_plan_measures_columns(const covt_plan* plan, covt_measures_info* out); /* tile order, num_geometry_columns */
int covt_plan_measures_descs(const covt_plan* plan, covt_measures_desc* out);   /* launch order (= covt_plan_geometry_descs) */

/* Measures of every assembled geometry column on `hip_stream`, after covt_assemble_geometry_device on the
 * same stream: d_decoded the decode output (GeometryTypes are read from it at covt_geom_desc.in_off[0]),
 * d_gdesc / d_asm / d_gres the assembly's descriptors, output and results, d_mdesc the measures descriptors
 * (same order), d_measures an output buffer of covt_plan_measures_bytes bytes, d_mres n_columns results (same
 * order).  Asynchronous; allocates nothing and writes every output element exactly once, so it can be
 * captured in a HIP graph as it is and its result does not depend on scheduling. */
int covt_geometry_measures_device(const uint8_t* d_decoded, const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                                  const covt_geom_result* d_gres, const covt_measures_desc* d_mdesc,
                                  int64_t n_columns, uint8_t* d_measures, covt_measures_result* d_mres,
                                  void* hip_stream);

/* Convenience: H2D + decode + assembly + measures + D2H of the whole plan on the current device.
 * host_measures: covt_plan_measures_bytes bytes; host_mres: one result per column in tile order. */
int covt_plan_measures_host(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, uint8_t* host_measures,
                            covt_measures_result* host_mres);

/* ---------------------------------------------------------------------------
 * Georeferenced geometry: the WKB values and the bounding boxes in a coordinate reference system instead of
 * tile pixels, so the columns of many tiles share one table, the bbox column prunes across tiles and a
 * GeoParquet writer can name a CRS.  A column's transform maps its assembled int32 pixel (px, py), converted
 * exactly to float64, where the plain passes convert it:
 *
 *   COVT_GEO_IDENTITY    X = px, Y = py                                   (the plain passes' output)
 *   COVT_GEO_AFFINE      X = ox + sx*px, Y = oy + sy*py
 *   COVT_GEO_AFFINE_LAT  X = ox + sx*px, t = oy + sy*py, Y = atan(sinh(t)) * (180/PI)
 *
 * The container does not hold a tile's address, so the caller supplies z/x/y; the layer's extent E comes
 * from its header (covt_plan_geometry_extents).  With W = 20037508.342789244 (pi * 6378137), PI the float64
 * nearest pi and n = 2^z as a double, covt_geo_transform gives
 *
 *   crs                     kind        sx               ox                   sy                oy
 *   COVT_CRS_TILE           IDENTITY    0                0                    0                 0
 *   COVT_CRS_WEB_MERCATOR   AFFINE      (2*W) / (n*E)    (2*W) * (x/n) - W    -sx               W - (2*W) * (y/n)
 *   COVT_CRS_CRS84          AFFINE_LAT  360.0 / (n*E)    360.0 * (x/n) - 180  -(2*PI) / (n*E)   PI - (2*PI) * (y/n)
 *
 * (EPSG:3857 metres; OGC:CRS84 longitude / latitude degrees, GeoParquet's default CRS.)  Everything is
 * evaluated in float64 in the order written, one rounding per operation and no fused multiply-add, on the
 * host and on the device.  So the table, every AFFINE coordinate and every longitude are bit-exact against
 * the same expressions in any IEEE-754 float64 arithmetic (numpy, Java); only the latitude goes through the
 * device's sinh and atan and agrees with another libm to a few ulp (tests hold it to 1e-9 degrees).
 * Valid input: 0 <= z <= 30, 0 <= x, y < 2^z, extent >= 1, a known crs; anything else is
 * COVT_ERR_INVALID_ARG.
 *
 * A projected WKB value has the byte count and offsets of the plain one (no SRID is written); only its
 * coordinate doubles differ.  A projected box is, per axis, fmin / fmax of the transformed ends of the int32
 * box (sy < 0 flips y, no sign test), the column extent likewise; a feature or column without a coordinate
 * stays the quiet NaN 0x7FF8000000000000.
 * Statuses of the projected passes: those of the plain passes, and a column whose kind is above
 * COVT_GEO_AFFINE_LAT or whose bit is missing from `kinds` gets COVT_ERR_INVALID_ARG (n_bytes 0 / n_empty 0,
 * extent NaN, slice untouched).  `kinds` with a bit above bit 2 makes the call return COVT_ERR_INVALID_ARG.
 * ------------------------------------------------------------------------- */
#define COVT_CRS_TILE 0         /* identity: tile-local, the plain passes' output */
#define COVT_CRS_WEB_MERCATOR 1 /* EPSG:3857, metres */
#define COVT_CRS_CRS84 2        /* OGC:CRS84 lon/lat degrees, GeoParquet's default CRS */

#define COVT_GEO_IDENTITY 0
#define COVT_GEO_AFFINE 1     /* X = ox + sx*px, Y = oy + sy*py */
#define COVT_GEO_AFFINE_LAT 2 /* X as AFFINE; t = oy + sy*py; Y = atan(sinh(t)) * (180/pi) */

/* One column's transform (40 bytes); a table of them is parallel to covt_geom_desc (launch order). */
typedef struct covt_geo_xform {
    double sx, ox, sy, oy;
    int32_t kind, reserved;
} covt_geo_xform;

/* The transform of tile z/x/y for a layer of `extent` pixels a side (pure host arithmetic). */
int covt_geo_transform(int32_t crs, int32_t z, int32_t x, int32_t y, int32_t extent, covt_geo_xform* out);

/* The extent of every geometry column's layer as its header states it, in tile order
 * (num_geometry_columns values; -1 where the header's value does not fit int32). */
int covt_plan_geometry_extents(const covt_plan* plan, int32_t* out);

/* The transform table of a plan for `crs`: tile_zxy holds z, x, y of every tile of the plan (3 per tile);
 * out gets num_geometry_columns entries in launch order (column c's at its covt_geom_info.desc_index), *kinds
 * the OR of 1u << kind over them.  An invalid address of a tile with a geometry column, or an extent < 1 on
 * one, is COVT_ERR_INVALID_ARG. */
int covt_plan_geo_transforms(const covt_plan* plan, int32_t crs, const int32_t* tile_zxy, covt_geo_xform* out,
                             uint32_t* kinds);

/* covt_geometry_wkb_device / covt_geometry_bbox_device with a transform per column: d_xf has n_columns
 * entries in d_gdesc order, `kinds` is the caller's promise of the kinds in it (the OR of 1u << kind), which
 * lets the launch leave the latitude code out when bit 2 is clear.  Asynchronous, no scratch, capturable. */
int covt_geometry_wkb_projected_device(const uint8_t* d_decoded, const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                                       const covt_geom_result* d_gres, const covt_wkb_desc* d_wdesc,
                                       int64_t n_columns, uint8_t* d_wkb, covt_wkb_result* d_wres,
                                       const covt_geo_xform* d_xf, uint32_t kinds, void* hip_stream);
int covt_geometry_bbox_projected_device(const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                                        const covt_geom_result* d_gres, const covt_bbox_desc* d_bdesc,
                                        int64_t n_columns, uint8_t* d_bbox, covt_bbox_result* d_bres,
                                        const covt_geo_xform* d_xf, uint32_t kinds, void* hip_stream);

/* covt_plan_wkb_host / covt_plan_bbox_host in `crs` (tile_zxy as covt_plan_geo_transforms; it may be null
 * for COVT_CRS_TILE).  Buffers and records are those of the plain entry points. */
int covt_plan_wkb_projected_host(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, int32_t crs,
                                 const int32_t* tile_zxy, uint8_t* host_wkb, covt_wkb_result* host_wres);
int covt_plan_bbox_projected_host(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, int32_t crs,
                                  const int32_t* tile_zxy, uint8_t* host_bbox, covt_bbox_result* host_bres);

/* ---------------------------------------------------------------------------
 * Feature selection: filtering the rows of a geometry column where the data is.  From a keep mask per feature
 * the pass writes the selection vector and the compacted WKB column (an Arrow `binary` column of the kept
 * values); a small predicate pass writes that mask from the bounding boxes and the measures (the viewport query
 * "features whose box meets this window", the per-zoom size cut "drop what this zoom cannot show"), or the
 * caller writes it.  Per geometry column one slice (16-byte aligned start) in the select buffer, every member
 * starting 16-byte aligned:
 *
 *   mask[n_features] uint8 | sel[n_features] int32 | offsets[n_features + 1] int32 | bytes[byte_cap]
 *
 * byte_cap is the column's WKB byte_cap: the output never exceeds the input, so there is no capacity status.
 * The input is the column's WKB column (wkb_offsets, wkb_bytes, covt_wkb_result).  With K = { f : mask[f] != 0 }
 * (any non-zero byte keeps a feature) and k_0 < k_1 < ... its members:
 *
 *   sel[j] = k_j
 *   offsets[0] = 0, offsets[j + 1] = offsets[j] + (wkb_offsets[k_j + 1] - wkb_offsets[k_j])
 *   bytes[offsets[j] .. offsets[j + 1]) = WKB value k_j, unchanged
 *   covt_select_result: n_selected = |K|, n_bytes = offsets[n_selected]
 *
 * Not written: sel[j] for j >= n_selected, offsets[j] for j > n_selected, bytes past n_bytes, and the mask (the
 * pass's input).  Every output element is written exactly once and no atomics are used, so the same input
 * gives the same bytes every time.  The fixed-width companions (ids, boxes, measures, property values) of the
 * kept features are array[sel[0 .. n_selected)].
 * Statuses: a column whose WKB result is not COVT_OK gets that status, n_selected 0, n_bytes 0 and nothing else
 * of its slice written (COVT_GEOM_TOO_LARGE arrives this way as COVT_ERR_INVALID_ARG); a descriptor flagged
 * COVT_SELECT_TOO_LARGE (set exactly where COVT_WKB_TOO_LARGE is) or whose n_features or byte_cap is not the WKB
 * descriptor's -> COVT_ERR_INVALID_ARG, likewise.  wkb_offsets no WKB pass writes (not nondecreasing inside
 * [0, covt_wkb_result.n_bytes]) are read clamped to that range, so no access leaves the two slices; if the kept
 * lengths then sum past n_bytes the column gets COVT_ERR_COUNT_MISMATCH (n_selected 0, n_bytes 0, sel and
 * offsets unspecified, no byte of `bytes` written).
 *
 * The predicate.  For feature f, with the column's bounding-box arrays xmin, ymin, xmax, ymax and its measures
 * area, length:
 *   xmin[f] is NaN (the feature has no coordinate): mask[f] = (flags & COVT_SELECT_KEEP_EMPTY) ? 1 : 0, and no
 *     other test applies;
 *   otherwise mask[f] = W && S, where
 *   W = true without COVT_SELECT_WINDOW, else xmin[f] <= window[2] && xmax[f] >= window[0] &&
 *       ymin[f] <= window[3] && ymax[f] >= window[1]   (window = xmin, ymin, xmax, ymax; closed intervals) &&
 *       window[0] <= window[2] && window[1] <= window[3]   (an inverted window selects nothing, also of a box
 *       that spans both its ends);
 *   S = true without COVT_SELECT_MIN_SIZE, else area[f] >= min_area || length[f] >= min_length ||
 *       (area[f] == 0.0 && length[f] == 0.0)   (features without extent, points for instance, are not judged
 *       by size).
 * Plain IEEE comparisons, so the mask is bit-exact against the same expressions anywhere.  The window is in
 * whatever space the bounding-box buffer was computed in (tile pixels, or the CRS of the projected pass); the
 * measures, and so min_area and min_length, are always tile pixels.  A column whose bounding-box result, or
 * with COVT_SELECT_MIN_SIZE its measures result, is not COVT_OK, or whose bounding-box / measures descriptor
 * does not have the select descriptor's n_features, gets an all-zero mask; the caller sees those statuses in
 * the bounding-box and measures results.
 * A NaN in window, min_area or min_length, an unknown flag bit or a wrong `size` makes a call return
 * COVT_ERR_INVALID_ARG.
 * Out of scope: compacted copies of the fixed-width columns (sel indexes them), clipping to the window, any
 * spatial index.  Predicates over property values are the where pass ("Property predicates" below), which
 * writes these masks or ANDs into them.
 * ------------------------------------------------------------------------- */
#define COVT_SELECT_TOO_LARGE 0x1 /* covt_select_desc.flags: set exactly where COVT_WKB_TOO_LARGE is */

#define COVT_SELECT_WINDOW 0x1u     /* covt_select_pred.flags: keep features whose box meets `window` */
#define COVT_SELECT_MIN_SIZE 0x2u   /* ... whose area or length reaches min_area / min_length (or has no extent) */
#define COVT_SELECT_KEEP_EMPTY 0x4u /* ... and the features without a coordinate */

/* One device-resident select column entry (24 bytes), parallel to covt_geom_desc (launch order). */
typedef struct covt_select_desc {
    int64_t off;      /* byte offset of the column's slice in the select buffer (16-byte aligned) */
    int64_t byte_cap; /* bytes the slice's `bytes` member holds (= covt_wkb_desc.byte_cap) */
    int32_t n_features, flags;
} covt_select_desc;

/* Per-column select result written by the kernels (16 bytes). */
typedef struct covt_select_result {
    int32_t status, n_selected; /* n_selected, n_bytes: 0 unless status is COVT_OK */
    int64_t n_bytes;
} covt_select_result;

/* Host-visible select column record of a plan, in tile order (40 bytes); column c belongs to geometry column c
 * (covt_geom_info). */
typedef struct covt_select_info {
    int32_t tile, layer, n_features, desc_index; /* desc_index: row in the launch-ordered descriptors */
    int64_t off, byte_cap;
    int32_t flags, reserved;
} covt_select_info;

/* The predicate of covt_select_predicate_device (56 bytes). */
typedef struct covt_select_pred {
    uint32_t size, flags; /* size: sizeof(covt_select_pred), set by covt_select_pred_init */
    double window[4];     /* xmin, ymin, xmax, ymax, in the space of the bounding-box buffer */
    double min_area, min_length; /* tile pixels */
} covt_select_pred;
void covt_select_pred_init(covt_select_pred* pred); /* size set, no flags, window and minima 0 */

int64_t covt_plan_select_bytes(const covt_plan* plan); /* size of the select buffer */
int covt_plan_select_columns(const covt_plan* plan, covt_select_info* out); /* tile order, num_geometry_columns */
int covt_plan_select_descs(const covt_plan* plan, covt_select_desc* out);   /* launch order (= covt_plan_geometry_descs) */

/* The masks of every column on `hip_stream`, after the bounding-box pass (and with COVT_SELECT_MIN_SIZE the
 * measures pass) on the same stream: d_bdesc / d_bbox / d_bres and d_mdesc / d_measures / d_mres those passes'
 * descriptors, buffers and results (the measures' three may be null without COVT_SELECT_MIN_SIZE), d_sdesc the
 * select descriptors (same order), `pred` in host memory (read before the call returns), d_select the select
 * buffer of covt_plan_select_bytes bytes, 16-byte aligned.  Asynchronous, no scratch, capturable. */
int covt_select_predicate_device(const covt_bbox_desc* d_bdesc, const uint8_t* d_bbox, const covt_bbox_result* d_bres,
                                 const covt_measures_desc* d_mdesc, const uint8_t* d_measures,
                                 const covt_measures_result* d_mres, const covt_select_desc* d_sdesc,
                                 int64_t n_columns, const covt_select_pred* pred, uint8_t* d_select, void* hip_stream);

/* Selection vectors and compacted WKB of every column on `hip_stream`, after the WKB pass and whatever wrote
 * the masks on the same stream (a caller may write its own masks into the slices, from a property column for
 * instance): d_wdesc / d_wkb / d_wres the WKB pass's descriptors, buffer and results, d_sdesc the select
 * descriptors (same order), d_select the select buffer (16-byte aligned), d_sres n_columns results (same
 * order).  A scan of (kept count, kept bytes), then a gather copy over the output bytes.  Asynchronous, no
 * scratch, capturable. */
int covt_geometry_select_device(const covt_wkb_desc* d_wdesc, const uint8_t* d_wkb, const covt_wkb_result* d_wres,
                                const covt_select_desc* d_sdesc, int64_t n_columns, uint8_t* d_select,
                                covt_select_result* d_sres, void* hip_stream);

/* Convenience: H2D + decode + assembly + WKB and bounding boxes in `crs` (tile_zxy as covt_plan_geo_transforms;
 * it may be null for COVT_CRS_TILE) + measures with COVT_SELECT_MIN_SIZE + predicate + select + D2H of the whole
 * plan on the current device.  host_select: covt_plan_select_bytes bytes; host_sres: one result per column in
 * tile order. */
int covt_plan_select_host(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, int32_t crs,
                          const int32_t* tile_zxy, const covt_select_pred* pred, uint8_t* host_select,
                          covt_select_result* host_sres);

/* ---------------------------------------------------------------------------
 * Geometry simplification: a cheaper version of every feature for a lower zoom, what PostGIS ST_AsMVTGeom and
 * tippecanoe do before they serialise: snap the coordinates to the target zoom's pixel grid (ST_SnapToGrid),
 * drop the vertices that now repeat their predecessor (ST_RemoveRepeatedPoints), and empty the rings and lines
 * that collapsed below what a reader accepts.  Integer arithmetic throughout, so the result is exact.
 *
 * Input: an assembled column (n features, P parts, R rings, V coordinates), the types t_f of its decoded
 * GeometryTypes stream (POINT 0, LINESTRING 1, POLYGON 2, MULTIPOINT 3, MULTILINESTRING 4, MULTIPOLYGON 5) and a
 * shift s in [0, COVT_SIMPLIFY_MAX_SHIFT]: the grid cell is 2^s tile pixels, s = source zoom - target zoom.
 *
 *   Snap.  snap(v) = min((((int64)v + h) >> s) << s, M) with h = s ? 2^(s-1) : 0, M = (INT32_MAX >> s) << s and
 *     >> arithmetic (floor): round half up to the grid; a value that would round past the int32 range snaps to
 *     the largest grid value that fits.  q_i = (snap(x_i), snap(y_i)).
 *   Keep.  Ring r covers the coordinates [a, b), a = ring_offsets[r], b = ring_offsets[r + 1]; t is the type of
 *     the ring's feature.  For t in {0, 3} every coordinate is kept; for any other t coordinate i is kept iff
 *     i == a or q_i != q_{i-1}.  The rule is local, so the kept sequence has no two equal neighbours, and a
 *     closed ring stays closed (its last kept value is q_{b-1} = q_a).  k_r is the number kept in ring r.
 *   Collapse.  t in {1, 4}: ring r is collapsed if k_r < 2.  t in {2, 5}: collapsed if k_r < 4 (JTS WKBReader
 *     rejects linear rings of 1 to 3 points and lines of 1 point; it accepts 0), and if the first ring of r's
 *     part is collapsed, every ring of that part is: a hole cannot outlive its shell (so an input part whose
 *     first ring is already empty loses its holes, also at s = 0).  k'_r = 0 for a collapsed ring, else k_r.
 *   Output.  An assembled column of the same shape in the column's slice of the simplify buffer:
 *     geometry_offsets[n + 1] and part_offsets[P + 1] copied, ring_offsets'[0] = 0, ring_offsets'[r + 1] =
 *     ring_offsets'[r] + k'_r, coords' the kept q_i of the non-collapsed rings in input order, and a
 *     covt_geom_result {status, num_parts = P, num_rings = R, num_coords = ring_offsets'[R]}.  Parts and rings
 *     are never removed, only emptied, so feature numbering and the number of rows stay.  A feature left
 *     without a coordinate is downstream what the other products define: num_coords 0, a NaN box, dropped by
 *     the select predicate unless COVT_SELECT_KEEP_EMPTY is set.
 *
 * Per column one slice (16-byte aligned start, every member padded to 16 bytes):
 *
 *   geometry_offsets[n + 1] | part_offsets[part_cap + 1] | ring_offsets[ring_cap + 1] | coords[2 * coord_cap]
 *   | scratch (a kept count per ring and per chunk of coordinates; contents unspecified)
 *
 * sized by one layout rule from the geometry column's capacities; the output never exceeds the input, so there
 * is no capacity status.  covt_plan_simplified_geometry_descs gives the geometry descriptors with out_off[0..3]
 * pointing into the simplify buffer: with that table, the simplify buffer as d_asm and the simplify results as
 * d_gres every pass that reads an assembled column (WKB, bounding boxes, measures, their projected forms, and
 * select after them) runs on the simplified column unchanged, with its own descriptors unchanged (capacities
 * only shrink).
 *
 * The pass is idempotent; s = 0 removes only exact repeats and collapses.  Every element of the output is
 * written exactly once; there are no atomics and no allocation, so the pass can be captured in a HIP graph as
 * it is and its bytes do not depend on scheduling.  Not written: ring_offsets' past R + 1, part_offsets past
 * P + 1, coords' past num_coords, the padding, and the whole slice of a failed column (its scratch included).
 * Offsets are read clamped as every product reads them, and every destination is checked against the slice:
 * whatever the input holds, no access leaves the slices.
 * Statuses: a column whose assembly result is not COVT_OK gets that status (counts 0); COVT_GEOM_TOO_LARGE,
 * COVT_SIMPLIFY_TOO_LARGE or a descriptor that does not match the geometry descriptor's capacities ->
 * COVT_ERR_INVALID_ARG; a per-column shift outside the range -> COVT_ERR_INVALID_ARG for that column; a uniform
 * shift outside it makes the call return COVT_ERR_INVALID_ARG.
 * Out of scope: Douglas-Peucker or Visvalingam, removal of collinear vertices or spikes, repair of the
 * self-intersections snapping can create, clipping, the Java binding.
 * ------------------------------------------------------------------------- */
#define COVT_SIMPLIFY_TOO_LARGE 0x1 /* covt_simplify_desc.flags: assembly refuses the column (COVT_GEOM_TOO_LARGE) */
#define COVT_SIMPLIFY_MAX_SHIFT 30

/* One device-resident simplify column entry (32 bytes), parallel to covt_geom_desc (launch order). */
typedef struct covt_simplify_desc {
    int64_t off; /* byte offset of the column's slice in the simplify buffer (16-byte aligned) */
    int32_t n_features, flags;
    int32_t part_cap, ring_cap, coord_cap, reserved; /* = covt_geom_desc's: what the slice was sized for */
} covt_simplify_desc;

/* Host-visible simplify column record of a plan, in tile order (40 bytes); column c belongs to geometry column
 * c (covt_geom_info). */
typedef struct covt_simplify_info {
    int32_t tile, layer, n_features, desc_index; /* desc_index: row in the launch-ordered descriptors */
    int64_t off;
    int32_t flags, part_cap, ring_cap, coord_cap;
} covt_simplify_info;

int64_t covt_plan_simplify_bytes(const covt_plan* plan); /* size of the simplify buffer */
int covt_plan_simplify_columns(const covt_plan* plan, covt_simplify_info* out); /* tile order, num_geometry_columns */
int covt_plan_simplify_descs(const covt_plan* plan, covt_simplify_desc* out);   /* launch order (= covt_plan_geometry_descs) */
/* covt_plan_geometry_descs with out_off[0..3] pointing into the simplify buffer (in_off, capacities unchanged). */
int covt_plan_simplified_geometry_descs(const covt_plan* plan, covt_geom_desc* out);
/* Per-tile shifts (n_tiles entries) -> per-column shifts in launch order (num_geometry_columns entries), as
 * covt_plan_geo_transforms does for transforms.  Values are passed through; the pass checks them per column. */
int covt_plan_simplify_shifts(const covt_plan* plan, const int32_t* tile_shift, int32_t* out);

/* Simplify every assembled geometry column on `hip_stream`, after covt_assemble_geometry_device on the same
 * stream: d_decoded the decode output (GeometryTypes are read from it), d_gdesc / d_asm / d_gres the assembly's
 * descriptors, output and results, d_sdesc the simplify descriptors (same order), `shift` for every column or,
 * if d_shift is not null, d_shift[c] for column c (launch order), d_simplify the simplify buffer of
 * covt_plan_simplify_bytes bytes (16-byte aligned, not the assembly buffer), d_gres_out n_columns results (same
 * order).  Asynchronous; allocates nothing, capturable. */
int covt_geometry_simplify_device(const uint8_t* d_decoded, const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                                  const covt_geom_result* d_gres, const covt_simplify_desc* d_sdesc,
                                  int64_t n_columns, int32_t shift, const int32_t* d_shift, uint8_t* d_simplify,
                                  covt_geom_result* d_gres_out, void* hip_stream);

/* Convenience: H2D + decode + assembly + simplify + D2H of the whole plan on the current device.  `shift` for
 * every tile or, if tile_shift is not null, tile_shift[t] for tile t.  host_simplify: covt_plan_simplify_bytes
 * bytes; host_gres: one result per column in tile order. */
int covt_plan_simplify_host(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, int32_t shift,
                            const int32_t* tile_shift, uint8_t* host_simplify, covt_geom_result* host_gres);

/* While set (enabled != 0), covt_plan_wkb_host, _bbox_host, _measures_host, _select_host and their projected
 * forms run the simplify pass after the assembly and read the simplified column.  tile_shift (n_tiles entries,
 * copied) may be null: `shift` for every tile.  Unset by default.  COVT_ERR_INVALID_ARG for a shift out of range. */
int covt_plan_set_simplify(covt_plan* plan, int32_t enabled, int32_t shift, const int32_t* tile_shift);

/* ---------------------------------------------------------------------------
 * Geometry as MVT: per feature the payload of a Mapbox Vector Tile Feature.geometry (field 4: packed uint32
 * varints, the command stream of the MVT 2.1 specification, section 4.3) and its GeomType, what a tile server
 * sends to MapLibre, OpenLayers, QGIS or ogr2ogr.  A host-side writer (the Python package's mvt_layer_bytes)
 * wraps the values, ids and property columns into layers; nothing of the protobuf framing is made on the device.
 *
 * Input: an assembled column (n features, P parts, R rings, V coordinates, offsets read clamped as every product
 * reads them), the types t_f of its GeometryTypes stream and covt_mvt_options {flags, shift}.  All arithmetic is
 * integer, so every byte is exact.
 *
 *   Coordinates.  q_i = (x_i >> s, y_i >> s), an arithmetic shift, s = shift in [0, COVT_MVT_MAX_SHIFT]: s = 0 for
 *     a tile at the layer's extent; after simplify(s), s emits a tile of extent E >> s.  All below is over q.
 *   Varint.  A uint32 is written as a 1 to 5 byte LEB128 varint.  A parameter is zz(d) = (d << 1) ^ (d >> 31) of
 *     the int32 difference d between the vertex and the cursor, taken with two's-complement wrap-around, so a
 *     reader that sums mod 2^32 recovers q exactly.  The cursor is (0, 0) at the start of every feature and the
 *     last emitted vertex afterwards; ClosePath does not move it.  A command integer is (count << 3) | id with
 *     MoveTo 1, LineTo 2, ClosePath 7.
 *   POINT, MULTIPOINT (t 0, 3).  c the feature's coordinate count: nothing if c = 0, else MoveTo(c) and the c
 *     parameter pairs in column order.
 *   LINESTRING, MULTILINESTRING (t 1, 4).  Per ring of m coordinates [a, a + m), in order: nothing if m = 0; else
 *     MoveTo(1) e_0 and, if m > 1, LineTo(m - 1) e_1 .. e_{m-1}, e_j = q_{a+j}.
 *   POLYGON, MULTIPOLYGON (t 2, 5).  Per ring [a, b), m = b - a: closed = m >= 2 and q_{b-1} == q_a; k = m - closed;
 *     nothing if k = 0, else MoveTo(1) e_0, LineTo(k - 1) e_1 .. e_{k-1} if k > 1, ClosePath(1).  Without
 *     COVT_MVT_ORIENT e_j = q_{a+j}, the ring as stored.  With it, S_r is the int64 shoelace of "Geometry
 *     measures" over q (the sum over i in a .. b - 2 of x_i * y_{i+1} - x_{i+1} * y_i mod 2^64, read as int64); a
 *     ring is reversed iff it is closed and it is the first ring of its part with S_r < 0 or another ring of its
 *     part with S_r > 0; a reversed ring emits e_j = q_{b-1-j} (it still starts at q_a = q_{b-1}).  Rings with
 *     S_r = 0 and rings that are not closed are emitted as stored.  This is the winding rule of MVT 2.1:
 *     exterior rings positive, interior rings negative in tile coordinates; snapping can flip small rings.
 *   GeomType.  type[f] = 1 for t 0 or 3, 2 for t 1 or 4, 3 for t 2 or 5, whatever the value's length.
 *   A feature whose value is empty (no coordinate, or only empty rings) has offsets[f + 1] == offsets[f].
 *
 * Per column one slice of the mvt buffer (16-byte aligned start, every member padded to 16 bytes):
 *
 *   type[n] uint8 | offsets[n + 1] int32 | bytes[byte_cap] | scratch (contents unspecified)
 *
 * byte_cap = 10 * coord_cap + 7 * ring_cap + 5 * n_features always suffices (a coordinate at most two 5-byte
 * varints, a ring at most MoveTo 1 + LineTo 5 + ClosePath 1, a point feature's MoveTo at most 5), so there is no
 * capacity status.  A column assembly refuses, or a capacity above INT32_MAX, gets COVT_MVT_TOO_LARGE.
 *
 * Result per column: covt_mvt_result {status, n_empty (features with an empty value), n_bytes = offsets[n]; both
 * 0 unless the status is COVT_OK}.  Every element of the output is written exactly once; there are no atomics
 * and no allocation, so the pass can be captured in a HIP graph as it is and its bytes do not depend on
 * scheduling.  Not written: offsets past n + 1, bytes past n_bytes, the padding, and the whole slice of a failed
 * column.  Every destination is checked against the slice: whatever the input holds, no access leaves the slices.
 * The values are defined, and free of scheduling, for a well-formed column, which is what assembly and simplify
 * write: offsets nondecreasing, every ring inside a part of a feature.  A column that is not (rings no part
 * covers, say) is still read and written inside its slices, but its bytes, offsets and n_bytes are unspecified.
 * Statuses: a column whose geometry result is not COVT_OK gets that status; COVT_GEOM_TOO_LARGE,
 * COVT_MVT_TOO_LARGE or a descriptor whose capacities are not the geometry descriptor's -> COVT_ERR_INVALID_ARG
 * for that column; a shift outside the range, an unknown flag bit or a wrong `size` makes the call return
 * COVT_ERR_INVALID_ARG.
 * Out of scope: clipping, compaction of selected features on the device, the protobuf layer, gzip, the Java
 * binding.
 * ------------------------------------------------------------------------- */
#define COVT_MVT_TOO_LARGE 0x1 /* covt_mvt_desc.flags: assembly refuses the column, or its capacity passes INT32_MAX */
#define COVT_MVT_ORIENT 0x1    /* covt_mvt_options.flags: wind polygon rings as MVT 2.1 asks */
#define COVT_MVT_MAX_SHIFT 30

/* Options of a call (16 bytes): host memory, read before the call returns. */
typedef struct covt_mvt_options {
    uint32_t size;  /* sizeof(covt_mvt_options) */
    uint32_t flags; /* COVT_MVT_ORIENT */
    int32_t shift, reserved;
} covt_mvt_options;
void covt_mvt_options_init(covt_mvt_options* opts); /* size set, no flags, shift 0 */

/* One device-resident mvt column entry (32 bytes), parallel to covt_geom_desc (launch order). */
typedef struct covt_mvt_desc {
    int64_t off;      /* byte offset of the column's slice in the mvt buffer (16-byte aligned) */
    int64_t byte_cap; /* capacity of bytes[] */
    int32_t n_features, flags;
    int32_t ring_cap, coord_cap; /* = covt_geom_desc's: what the slice was sized for */
} covt_mvt_desc;

/* Host-visible mvt column record of a plan, in tile order (48 bytes); column c belongs to geometry column c.
 * type[] is at off, offsets[] at off + align16(n_features), bytes[] after the offsets' align16(4 (n_features + 1)). */
typedef struct covt_mvt_info {
    int32_t tile, layer, n_features, desc_index; /* desc_index: row in the launch-ordered descriptors */
    int64_t off, byte_cap;
    int32_t flags, ring_cap, coord_cap, reserved;
} covt_mvt_info;

typedef struct covt_mvt_result {
    int32_t status, n_empty;
    int64_t n_bytes;
} covt_mvt_result;

int64_t covt_plan_mvt_bytes(const covt_plan* plan); /* size of the mvt buffer */
int covt_plan_mvt_columns(const covt_plan* plan, covt_mvt_info* out); /* tile order, num_geometry_columns */
int covt_plan_mvt_descs(const covt_plan* plan, covt_mvt_desc* out);   /* launch order (= covt_plan_geometry_descs) */

/* Encode every assembled geometry column on `hip_stream`, after covt_assemble_geometry_device on the same stream:
 * d_decoded the decode output (GeometryTypes are read from it), d_gdesc / d_asm / d_gres the assembly's
 * descriptors, output and results (or covt_plan_simplified_geometry_descs, the simplify buffer and the simplify
 * results: the simplified column), d_mvdesc the mvt descriptors (same order), d_mvt the mvt buffer of
 * covt_plan_mvt_bytes bytes (16-byte aligned), d_mvres n_columns results (same order).  Asynchronous; allocates
 * nothing, capturable. */
int covt_geometry_mvt_device(const uint8_t* d_decoded, const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                             const covt_geom_result* d_gres, const covt_mvt_desc* d_mvdesc, int64_t n_columns,
                             const covt_mvt_options* opts, uint8_t* d_mvt, covt_mvt_result* d_mvres, void* hip_stream);

/* Convenience: H2D + decode + assembly (+ simplify while covt_plan_set_simplify is set) + mvt + D2H of the whole
 * plan on the current device.  host_mvt: covt_plan_mvt_bytes bytes; host_mvres: one result per column in tile
 * order. */
int covt_plan_mvt_host(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, const covt_mvt_options* opts,
                       uint8_t* host_mvt, covt_mvt_result* host_mvres);

/* ---------------------------------------------------------------------------
 * Property columns: the GPU replacement for
 * CovtParser.decodePropertyColumn (CovtParser.java:276-354) and getStringDictionary (:367-377).
 * A plan created with COVT_PLAN_PROPERTIES also plans every property column: its present / data /
 * length streams join the decode launch (column_kind 2 in covt_stream_info, stream_type = the
 * StreamType PRESENT 0 / DATA 1 / LENGTH 2), and covt_materialize_properties_device turns them into
 * Arrow-style columns, one per (sub)column:
 *
 *   validity[ceil(n/8)]   present bits, LSB first (BitSet.valueOf); all set without a present stream
 *   values                BOOLEAN: bitmap[ceil(n/8)];  INT64: int64[n];  FLOAT: float32[n];
 *                         STRING: int32 dictionary index [n]  (absent slots hold 0)
 *   dict_offsets[n_dict+1], dict_bytes   STRING: Arrow string offsets + UTF-8 bytes of the dictionary
 *
 * Java's List<Optional> per feature is validity bit i ? value i : empty.  Localized dictionary
 * columns (Gen C LOCALIZED_DICTIONARY, which Java rejects with IllegalArgumentException) are
 * decoded as format truth: one STRING sub-column per language stream, sharing the column's
 * dictionary (written once, by the sub-column flagged COVT_PROP_DICT_OWNER).  Gen C boolean columns
 * with a present stream store only the present values' bits (data numValues = present count).
 * INT_64 varint columns follow id_mode: COVT_ID_JAVA = the 4-byte-capped int decode widened to long
 * (CovtParser.java:304-312), COVT_ID_FORMAT = 64-bit zigzag varints (what the writer emits).
 * Statuses follow Java's order: a failed source stream first, then the dictionary (negative length
 * -> COUNT_MISMATCH, strings past the dictionary stream -> TRUNCATED), then the feature loop
 * (a present bit without a data value or a dictionary index out of range -> COUNT_MISMATCH).
 * ------------------------------------------------------------------------- */
#define COVT_PLAN_PROPERTIES 0x1u /* covt_plan_create_ex flag */

#define COVT_PROP_BOOLEAN 0
#define COVT_PROP_INT64 1
#define COVT_PROP_FLOAT 2
#define COVT_PROP_STRING 3

#define COVT_PROP_DICT_OWNER 0x1  /* this sub-column writes the dictionary offsets and bytes */
#define COVT_PROP_DENSE_BOOL 0x2  /* BOOLEAN data holds the present values' bits only (Gen C) */
#define COVT_PROP_UNSUPPORTED 0x4 /* data type / missing stream Java rejects: UNSUPPORTED_ENCODING */
#define COVT_PROP_DATA_SHORT 0x8  /* FLOAT data stream shorter than numValues * 4: TRUNCATED */
#define COVT_PROP_UNSUPPORTED_LATE 0x10 /* encoding Java rejects after decoding the present stream */

/* One device-resident property (sub)column entry (96 bytes). */
typedef struct covt_prop_desc {
    int64_t present_off; /* decode-output byte offset of the present bitset (-1: none, all valid) */
    int64_t data_off;    /* decode-output offset of the dense data (BOOLEAN bits, INT64 int64, STRING int32
                            indices); FLOAT: INPUT offset of the little-endian floats */
    int64_t length_off;  /* STRING: decode-output offset of the int32 dictionary lengths */
    int64_t dict_in_off; /* STRING: input offset of the dictionary bytes */
    int64_t out_off[4];  /* validity, values, dictionary offsets, dictionary bytes (16-byte aligned) */
    int32_t res[3];      /* decode-result rows of the present, data, length streams (-1: none) */
    int32_t n_features, n_data, n_dict, dict_bytes;
    int16_t type, flags; /* COVT_PROP_*, COVT_PROP_* flags */
} covt_prop_desc;

typedef struct covt_prop_result {
    int32_t status;  /* COVT_OK, a source stream's status, or a COVT_ERR_* of the materialization */
    int32_t n_valid; /* features with a value */
} covt_prop_result;

/* Host-visible property (sub)column record of a plan, in tile order (112 bytes). */
typedef struct covt_prop_info {
    int32_t tile, layer, column, type;          /* type: COVT_PROP_* or -1 (unsupported data type) */
    int32_t column_type, n_features, n_data, n_dict;
    int32_t lang, name_len, lang_len, dict_bytes; /* lang: language index of a localized sub-column, -1 */
    int32_t stream[3];                          /* tile-order stream index of present, data, length (-1) */
    int32_t desc_index;                         /* row in the launch-ordered property descriptors */
    int64_t name_off, lang_off;                 /* UTF-8 column / language names in the batch input (-1) */
    int64_t out_off[4];
} covt_prop_info;

/* covt_plan_create plus flags (COVT_PLAN_PROPERTIES), default options otherwise. */
int covt_plan_create_ex(const uint8_t* bytes, const uint64_t* tile_offsets, const uint64_t* tile_sizes,
                        int32_t n_tiles, int32_t format, int32_t id_mode, uint32_t flags, covt_plan** out);
/* covt_plan_create with explicit options (NULL: the defaults).  COVT_ERR_INVALID_ARG for an
 * options struct of the wrong size or out-of-range fields. */
int covt_plan_create_opts(const uint8_t* bytes, const uint64_t* tile_offsets, const uint64_t* tile_sizes,
                          int32_t n_tiles, int32_t format, int32_t id_mode, const covt_plan_options* opts,
                          covt_plan** out);
int64_t covt_plan_num_property_columns(const covt_plan* plan);
int64_t covt_plan_property_bytes(const covt_plan* plan); /* size of the property output buffer */
int covt_plan_property_columns(const covt_plan* plan, covt_prop_info* out); /* tile order */
int covt_plan_property_descs(const covt_plan* plan, covt_prop_desc* out);   /* launch order (largest first) */

/* Materialize every property column on `hip_stream` after the decode launch of the same plan:
 * d_in the batch input (dictionary bytes and floats are read from it), d_decoded / d_res the decode
 * output and launch-order results, d_pdesc the property descriptors, d_props an output buffer of
 * covt_plan_property_bytes bytes, d_pres n_columns results (in d_pdesc order).  Asynchronous. */
int covt_materialize_properties_device(const uint8_t* d_in, const uint8_t* d_decoded, const covt_stream_result* d_res,
                                       const covt_prop_desc* d_pdesc, int64_t n_columns, uint8_t* d_props,
                                       covt_prop_result* d_pres, void* hip_stream);

/* Scratch of the small-batch paths.  For batches of at most 4,096 columns covt_assemble_geometry_device
 * and covt_materialize_properties_device keep one device scratch block per (device, HIP stream) (about
 * 8.4 MB for assembly, 0.6 MB for properties), allocated and zeroed on the stream's first use and reused
 * by every later launch on it.  Each launch tags its look-back records with an epoch its own first kernel
 * advances in device memory, so launches captured in a HIP graph replay correctly -- under two rules: a
 * graph is replayed on its capture stream (or on streams ordered with it: replays of graphs that share a
 * capture stream must not overlap, they share one block's tickets and epoch), and the stream has run one
 * such launch before the capture (a block cannot be allocated while capturing: the launch then fails with
 * COVT_ERR_DEVICE).  A block used under a capture is pinned for the graph: it is never evicted and
 * covt_release_scratch frees it only with COVT_RELEASE_PINNED.  At most 16 unpinned blocks of each kind
 * are kept; beyond that the least recently used unpinned one is freed.  covt_release_scratch frees the
 * unpinned block of (current device, hip_stream), or every unpinned block when bit 0 of `all` is set, plus
 * the pinned ones matched the same way with COVT_RELEASE_PINNED (the caller promises that no graph
 * captured on them replays again), and returns how many it freed.  hipFree waits for the device, so no
 * launch still in flight uses a freed block; a caller that creates a stream per batch should release its
 * blocks before destroying the stream. */
#define COVT_RELEASE_PINNED 0x2
int covt_release_scratch(void* hip_stream, int all);
/* blocks currently held (assembly + properties) */
int64_t covt_scratch_blocks(void);

/* Convenience: H2D + decode + property materialization + D2H of the whole plan on the current device.
 * host_props: covt_plan_property_bytes bytes; host_pres: one result per (sub)column in tile order. */
int covt_plan_properties_host(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, uint8_t* host_props,
                              covt_prop_result* host_pres);

/* ---------------------------------------------------------------------------
 * Property predicates: the *where* pass.  A conjunction of clauses over named property (sub)columns, evaluated
 * per feature on the device over the materialized property columns (covt_materialize_properties_device), which
 * writes the keep masks covt_geometry_select_device consumes, or ANDs into them: `class in (motorway, trunk)`,
 * `rank <= 3`, `name:de is null`.
 *
 * The predicate (covt_where) is one flat POD, filled on the host (covt_where_init, covt_where_add_clause) and
 * copied to the device by the caller as it lies: clause headers, the literals of all clauses, and one text area
 * holding the clause names and the string literals.  Values per op: IS_NULL / NOT_NULL 0, EQ .. GE exactly 1,
 * IN / NOT_IN 1 .. COVT_WHERE_MAX_IN.  A literal carries a set of kinds and one value per kind; it compares only
 * with a column of one of its kinds.  covt_where_add_clause returns COVT_ERR_INVALID_ARG, and leaves *w byte for
 * byte as it was, for: a value with no kind bit (or an unknown one), a NaN d, an unknown op or flag, a wrong
 * number of values, a ninth clause, a 33rd value, text past COVT_WHERE_MAX_TEXT bytes, a *w that is not valid.
 *
 * Binding.  A clause names a (sub)column as Plan.property_name spells it: the column name, plus ':' + language
 * for a localized sub-column.  covt_where_bind is pure host code over the record arrays (a host plan's, or the
 * copies a device plan hands out): out[g.desc_index * COVT_WHERE_MAX_CLAUSES + k] = the desc_index of the first
 * property record, in tile order, with tile == g.tile, layer == g.layer and a full name bytewise equal to
 * clause k's name; -1 when none matches, and for the unused clause slots.  Names are read from `bytes` at
 * name_off / lang_off; a name that leaves [0, n_bytes) matches nothing.
 *
 * Truth of clause k for feature f of geometry column c, bound to property column p = bind[c * 8 + k]:
 *   Absent (p == -1, or validity bit f of p clear): IS_NULL true, NOT_NULL false, every other op true iff the
 *     clause has COVT_WHERE_NULL_MATCHES.
 *   Present: IS_NULL false, NOT_NULL true.  The other ops start from eq(v, L) and lt(v, L) between the value
 *     and a literal:
 *       BOOLEAN column: defined iff L has COVT_WHERE_BOOL; eq is v == (L.b != 0); no order.
 *       INT64 column: defined iff L has COVT_WHERE_INT; int64 comparisons with L.i.
 *       FLOAT column: defined iff L has COVT_WHERE_REAL; the float32 value widened exactly to double and
 *         compared with L.d by plain IEEE comparisons (a NaN value equals nothing and is ordered with nothing;
 *         (double)0.1f == 0.1 is false).
 *       STRING column: defined iff L has COVT_WHERE_STRING; eq iff the lengths and the bytes are equal, the
 *         entry being dict_bytes[dict_offsets[v] .. dict_offsets[v + 1]) with the offsets read clamped to
 *         [0, dict_bytes] (an inverted range is empty); an index outside [0, n_dict) equals nothing; no order.
 *     An undefined eq or lt is false.  EQ = eq(v, L0), NE = !EQ; LT = lt, LE = lt || eq, GT = lt(L0, v),
 *     GE = GT || eq (false where undefined, and for a NaN value); IN = any literal equal, NOT_IN = !IN.
 *   P[f] = the AND over the n_clauses clauses (no clause: true).  COVT_WHERE_WRITE: mask[f] = P;
 *   COVT_WHERE_AND: mask[f] = (mask[f] != 0 && P) ? 1 : 0.
 * Column rule.  The whole mask of column c becomes 0, in both modes, and status[c] gets the cause, when for some
 * clause k (the lowest such k wins): the bind entry lies outside [-1, n_prop_columns) -> COVT_ERR_INVALID_ARG;
 * the bound column's covt_prop_result.status is not COVT_OK -> that status; the bound column's descriptor
 * n_features differs from the select descriptor's -> COVT_ERR_INVALID_ARG.  A select descriptor flagged
 * COVT_SELECT_TOO_LARGE, or with n_features <= 0, writes no mask byte and gets status COVT_OK.
 *
 * The kernel reads the blob clamped to its own bounds (n_clauses <= 8, value ranges inside `values`, text ranges
 * inside `text`), dictionary indices and offsets clamped as above, and the property members as the layout rule
 * sizes them (every member padded to 16 bytes): whatever the buffers hold, no access leaves the property
 * slices, the blob, the bind table, the mask members and the status array.  Every mask byte of a live column is
 * written exactly once; no atomics, no scratch buffer, so the same input gives the same bytes and the pass can
 * be captured in a HIP graph as it is.
 * Out of scope: OR / NOT trees; string ordering or prefix match; mixed-kind numeric comparison (an INT-only
 * literal on a FLOAT column matches nothing, by the rule above); compacted copies of property columns; the Java
 * binding; building the bind table on the device.
 * ------------------------------------------------------------------------- */
#define COVT_WHERE_MAX_CLAUSES 8
#define COVT_WHERE_MAX_VALUES 32  /* over all clauses */
#define COVT_WHERE_MAX_TEXT 1024  /* bytes of clause names + string literals */
#define COVT_WHERE_MAX_IN 16      /* values of one IN / NOT_IN */

#define COVT_WHERE_EQ 0
#define COVT_WHERE_NE 1
#define COVT_WHERE_LT 2
#define COVT_WHERE_LE 3
#define COVT_WHERE_GT 4
#define COVT_WHERE_GE 5
#define COVT_WHERE_IN 6
#define COVT_WHERE_NOT_IN 7
#define COVT_WHERE_IS_NULL 8
#define COVT_WHERE_NOT_NULL 9

#define COVT_WHERE_BOOL 1u /* covt_where_value.kinds: a bit set */
#define COVT_WHERE_INT 2u
#define COVT_WHERE_REAL 4u
#define COVT_WHERE_STRING 8u

#define COVT_WHERE_NULL_MATCHES 1u /* covt_where_clause.flags: an absent value satisfies the clause */

#define COVT_WHERE_WRITE 0 /* mode: mask = P */
#define COVT_WHERE_AND 1   /* mode: mask = mask && P */

/* One literal of the blob (32 bytes): a value per kind it may be read as. */
typedef struct covt_where_value {
    int64_t i;                /* COVT_WHERE_INT */
    double d;                 /* COVT_WHERE_REAL (never NaN) */
    int32_t str_off, str_len; /* COVT_WHERE_STRING: bytes of covt_where.text */
    uint32_t kinds;
    int32_t b;                /* COVT_WHERE_BOOL: false iff 0 */
} covt_where_value;

/* One clause of the blob (32 bytes). */
typedef struct covt_where_clause {
    int32_t op;
    uint32_t flags;
    int32_t first_value, n_values; /* its literals: covt_where.values[first_value .. first_value + n_values) */
    int32_t name_off, name_len;    /* the (sub)column's name in covt_where.text */
    int32_t reserved[2];
} covt_where_clause;

/* The predicate (2320 bytes). */
typedef struct covt_where {
    uint32_t size, n_clauses, n_values, text_len; /* size: sizeof(covt_where), set by covt_where_init */
    covt_where_clause clauses[COVT_WHERE_MAX_CLAUSES];
    covt_where_value values[COVT_WHERE_MAX_VALUES];
    uint8_t text[COVT_WHERE_MAX_TEXT];
} covt_where;

/* A literal as covt_where_add_clause takes it (40 bytes): str points at str_len bytes in host memory. */
typedef struct covt_where_literal {
    uint32_t kinds;
    int32_t b;
    int64_t i;
    double d;
    const uint8_t* str;
    int32_t str_len, reserved;
} covt_where_literal;

void covt_where_init(covt_where* w); /* size set, no clause, everything else 0 */
int covt_where_add_clause(covt_where* w, const uint8_t* name, int32_t name_len, int32_t op, uint32_t flags,
                          const covt_where_literal* literals, int32_t n);
int covt_where_valid(const covt_where* w); /* 1: what covt_where_add_clause builds; 0 otherwise */

/* The bind table of `w` over geometry records ginfo[n_geom] and property records pinfo[n_props] (both in tile
 * order), names read from bytes[0, n_bytes): out holds n_geom * COVT_WHERE_MAX_CLAUSES entries.
 * COVT_ERR_INVALID_ARG for an invalid w, a null array or a desc_index outside [0, n_geom). */
int covt_where_bind(const covt_where* w, const covt_geom_info* ginfo, int64_t n_geom, const covt_prop_info* pinfo,
                    int64_t n_props, const uint8_t* bytes, uint64_t n_bytes, int32_t* out);
/* The same over a host plan's records; COVT_ERR_INVALID_ARG for a plan made without COVT_PLAN_PROPERTIES. */
int covt_plan_where_bind(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, const covt_where* w,
                         int32_t* out);

/* The where pass on `hip_stream`, after covt_materialize_properties_device and, with COVT_WHERE_AND, after
 * whatever wrote the masks, on the same stream: d_pdesc / d_props / d_pres the property descriptors, buffer
 * and results (n_prop_columns of them), d_sdesc the select descriptors of n_columns geometry columns (launch
 * order), d_where the blob and d_bind the bind table (n_columns * COVT_WHERE_MAX_CLAUSES) in device memory,
 * d_select the select buffer (16-byte aligned), d_status n_columns statuses in launch order (may be null).
 * Asynchronous, no scratch buffer, capturable. */
int covt_select_where_device(const covt_prop_desc* d_pdesc, const uint8_t* d_props, const covt_prop_result* d_pres,
                             int64_t n_prop_columns, const covt_select_desc* d_sdesc, int64_t n_columns,
                             const covt_where* d_where, const int32_t* d_bind, int32_t mode, uint8_t* d_select,
                             int32_t* d_status, void* hip_stream);
/* Dictionary entries up to which a STRING clause is evaluated through a match bitmap in LDS: which = 0 a
 * workgroup per column (batches of at most 4,096 columns), 1 a wave per column. */
int32_t covt_where_dict_bound(int32_t which);

/* Convenience: covt_plan_select_host with a property predicate: H2D + decode + assembly + property
 * materialization + WKB and bounding boxes in `crs` + the geometric predicate (pred not null) and the where
 * pass in AND mode, or (pred null) the where pass in WRITE mode + select + D2H.  host_where_status: one status
 * per column in tile order (may be null).  The plan must have been made with COVT_PLAN_PROPERTIES; honours
 * covt_plan_set_simplify. */
int covt_plan_select_where_host(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, int32_t crs,
                                const int32_t* tile_zxy, const covt_select_pred* pred, const covt_where* where,
                                uint8_t* host_select, covt_select_result* host_sres, int32_t* host_where_status);

/* ---------------------------------------------------------------------------
 * Geometry queries: the *query* pass.  For every feature of every assembled geometry column it decides one of
 * two exact relations with a closed, axis-aligned window in tile pixels, from the coordinates themselves, and
 * writes the keep masks covt_geometry_select_device consumes, or ANDs into them: what is under this pixel
 * within r pixels, what meets this viewport, what lies wholly inside it.  (COVT_SELECT_WINDOW of the
 * geometric predicate looks at the bounding box only: a prefilter.)
 *
 * The window is W = [wx0, wx1] x [wy0, wy1] = window[0 .. 3] = (wx0, wy0, wx1, wy1), int32, closed;
 * in(p) = wx0 <= x <= wx1 && wy0 <= y <= wy1; Q = (wx0, wy0).  A point query is wx0 = wx1, wy0 = wy1; a point
 * with tolerance r is the square of half-width r around it.  The window is always in tile pixels, whatever
 * CRS the boxes were computed in, as the measures are.
 *
 * Segment test.  meets(a, b) says whether the closed segment ab and W share a point:
 *   1. false if max(ax, bx) < wx0, or min(ax, bx) > wx1, or the same in y;
 *   2. otherwise true if in(a) or in(b);
 *   3. otherwise, for each of the four corners c of W, s = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax):
 *      true iff the four s are not all > 0 and not all < 0.
 * Crossing test.  cross(a, b) = ((ay > qy) != (by > qy)) && ((D > 0) == (by > ay)) with
 *   D = (qy - ay) * (bx - ax) - (qx - ax) * (by - ay).
 * Every difference of two int32 has 33 bits and every product 66: the signs are those of the exact integers,
 * no floating point.
 *
 * Per ring.  Ring r has the coordinates p_0 .. p_{m-1} as assembled (the closing vertex included, no implicit
 * closing edge, as in the measures).  Three bits:
 *   touch_r = m == 1 ? in(p_0) : OR over i <= m - 2 of meets(p_i, p_{i+1})      (m = 0: 0)
 *   out_r   = OR over all i of !in(p_i)
 *   par_r   = XOR over i <= m - 2 of cross(p_i, p_{i+1})
 * Per feature f of GeometryTypes ordinal t, the OR and XOR over all rings of all its parts:
 *   INTERSECTS_f = OR touch_r, or (t in {2, 5} and XOR par_r = 1).  (If no edge meets W, W lies wholly inside
 *     or outside every ring; even-odd of one point of W over the rings is then "in a shell and in no hole".)
 *   WITHIN_f = f has at least one coordinate and OR out_r = 0.  (W is convex: all vertices inside puts all
 *     edges and interiors inside.)
 * A feature without a coordinate gets 0 for both.  An inverted window (wx0 > wx1 or wy0 > wy1) gives 0 for
 * both for every feature.
 *
 * Predicate and masks.  P_f is INTERSECTS_f or WITHIN_f, whichever `relation` names.  COVT_WHERE_WRITE:
 * mask[f] = P_f; COVT_WHERE_AND: mask[f] = (mask[f] != 0) && P_f; the values are 0 or 1.
 * Column rule.  A column gets the status of the other products' precheck and, in both modes, an all-zero
 * mask, when its assembly result is not COVT_OK (that status), or its select descriptor is flagged
 * COVT_SELECT_TOO_LARGE, is misaligned (off negative or not a multiple of 16), or is planned for another feature
 * count than the assembly walked (COVT_ERR_INVALID_ARG).  (No byte is written at a negative off.)
 *
 * Scratch.  The pass is no product of its own: it writes into the select product's slice.  Its per-ring
 * scratch, one byte per ring (touch | out << 1 | par << 2), lives in the first ring_cap bytes (the geometry
 * descriptor's) of the slice's `bytes` member, which covt_geometry_select_device writes afterwards; byte_cap =
 * 9 (n + part_cap) + 4 ring_cap + 16 coord_cap always holds it, and a hand-made descriptor with byte_cap <
 * ring_cap gets COVT_ERR_INVALID_ARG by the column rule.  Between this pass and covt_geometry_select_device
 * the head of `bytes` is unspecified; no other byte of the slice outside `mask` is touched.
 * No atomics, every mask byte written exactly once, no allocation: the same input gives the same bytes and the
 * pass can be captured in a HIP graph as it is.
 * Out of scope: clipping to the window; queries in a CRS; distance to a feature; polygons as query shapes; a
 * nonzero fill rule; the Java binding.
 * ------------------------------------------------------------------------- */
#define COVT_QUERY_INTERSECTS 0
#define COVT_QUERY_WITHIN 1

typedef struct covt_select_query {
    uint32_t size;     /* sizeof(covt_select_query), set by covt_select_query_init */
    uint32_t flags;    /* 0 */
    int32_t relation;  /* COVT_QUERY_* */
    int32_t reserved;  /* 0 */
    int32_t window[4]; /* wx0, wy0, wx1, wy1 */
} covt_select_query;

void covt_select_query_init(covt_select_query* query); /* size set, INTERSECTS, the window (0, 0, 0, 0) */

/* The query pass on `hip_stream`, after the assembly (or covt_geometry_simplify_device: with the simplified
 * descriptors, buffer and results it runs on the simplified column unchanged) and, with COVT_WHERE_AND, after
 * whatever wrote the masks, on the same stream.  d_decoded / d_gdesc / d_asm / d_gres as the measures pass
 * takes them, d_sdesc the select descriptors (launch order), `query` in host memory, read before the call
 * returns; mode COVT_WHERE_WRITE or COVT_WHERE_AND; d_select the select buffer (16-byte aligned); d_status
 * n_columns statuses in launch order (may be null).  COVT_ERR_INVALID_ARG for a query with a wrong size, a
 * nonzero flags or reserved or an unknown relation, an unknown mode, a negative n_columns or a null array.
 * Asynchronous, capturable, allocates nothing. */
int covt_select_query_device(const uint8_t* d_decoded, const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                             const covt_geom_result* d_gres, const covt_select_desc* d_sdesc, int64_t n_columns,
                             const covt_select_query* query, int32_t mode, uint8_t* d_select, int32_t* d_status,
                             void* hip_stream);

/* Convenience: the select pipeline of covt_plan_select_where_host with the query pass as a third optional stage
 * after the geometric predicate (pred) and the where pass (where): in AND mode when one of them wrote the
 * masks, in WRITE mode when both are null -- then no boxes and no properties are computed.  At least one of the
 * three must be given; `where` needs a plan made with COVT_PLAN_PROPERTIES.  host_where_status /
 * host_query_status: one status per column in tile order (each may be null).  Honours covt_plan_set_simplify. */
int covt_plan_select_query_host(const covt_plan* plan, const uint8_t* bytes, uint64_t n_bytes, int32_t crs,
                                const int32_t* tile_zxy, const covt_select_pred* pred, const covt_where* where,
                                const covt_select_query* query, uint8_t* host_select, covt_select_result* host_sres,
                                int32_t* host_where_status, int32_t* host_query_status);

/* ---- Device-side plan ------------------------------------------------------------------------
 * covt_plan_create's Id / Geometry walk run on the GPU, for tiles already resident in HBM (the host
 * half of CovtParser.decodeCovt, CovtParser.java:53-133 / :574-652, without the round trip through
 * host memory).  d_bytes / n_bytes: the batch on the current device; d_tile_offsets / d_tile_sizes:
 * n_tiles uint64 each, on the device (a tile outside [0, n_bytes) gets COVT_ERR_INVALID_ARG as its
 * status).  The result is the host plan's layout exactly: streams in tile order with the same
 * covt_stream_info fields and 128-byte aligned output slices, descriptors in the same launch order
 * and families, including the split rule: with the same options, the long poles of a small batch are
 * cut into the same chunks (varint byte chunks, FastPFOR value chunks with their start states, ORC RLE
 * group chunks); geometry-column planning on request (covt_device_plan_geometry); property columns
 * with COVT_PLAN_PROPERTIES in opts->flags.  Multi-GPU shards stay with the host plan.
 * Runs on `hip_stream` and synchronises it: once for an Id / Geometry plan of more than
 * split_max_streams / 32 tiles (nothing splits there; the stream arrays are sized to 64 streams per tile
 * and the count is checked at the end -- a batch averaging more is redone with its counted size: three
 * syncs), otherwise twice (three times when it splits: the stream count and the descriptor count size the
 * arrays); COVT_PLAN_PROPERTIES adds one more (the property record count).  COVT_ERR_BAD_HEADER if the property walk fails a tile the Id / Geometry walk accepted (the
 * walkers diverged: never on well-formed or corrupted input that the host plan rejects the same way).
 * Limits and memory: a tile of 0x7ff00000 bytes or more gets COVT_ERR_INVALID_ARG as its status
 * (32-bit cursors; the host plan walks such tiles); besides the stream arrays the plan holds ~5 KiB
 * of per-tile walk slots on the device (128 stream records of 40 bytes per tile: ~0.5 GB at 100k
 * tiles) unless opts->device_walk != 0.  The arenas come from a per-device stream-ordered memory pool
 * that keeps up to 1 GiB of freed plan memory for the next plan (PyTorch's allocator does not see it);
 * covt_device_plan_pool_trim(device, keep_bytes) releases all but keep_bytes of it. */
typedef struct covt_device_plan covt_device_plan;
int covt_device_plan_create(const uint8_t* d_bytes, uint64_t n_bytes, const uint64_t* d_tile_offsets,
                            const uint64_t* d_tile_sizes, int32_t n_tiles, int32_t format, int32_t id_mode,
                            void* hip_stream, covt_device_plan** out);
/* the same with explicit options (NULL: the defaults; flags: 0 or COVT_PLAN_PROPERTIES) */
int covt_device_plan_create_opts(const uint8_t* d_bytes, uint64_t n_bytes, const uint64_t* d_tile_offsets,
                                 const uint64_t* d_tile_sizes, int32_t n_tiles, int32_t format, int32_t id_mode,
                                 const covt_plan_options* opts, void* hip_stream, covt_device_plan** out);
void covt_device_plan_destroy(covt_device_plan* plan);
int covt_device_plan_pool_trim(int device, uint64_t keep_bytes);
int64_t covt_device_plan_num_streams(const covt_device_plan* plan);
int64_t covt_device_plan_num_descs(const covt_device_plan* plan); /* = num_streams unless it splits */
int64_t covt_device_plan_output_bytes(const covt_device_plan* plan);
int covt_device_plan_totals(const covt_device_plan* plan, int64_t* in_bytes, int64_t* out_bytes, int64_t* vertices);
int covt_device_plan_family_counts(const covt_device_plan* plan, int64_t counts[COVT_NUM_FAMILIES]);
/* device arrays owned by the plan: num_descs descriptors (launch order), num_streams stream records
 * (tile order, desc_index = the stream's first descriptor), n_tiles statuses, and the stream index of
 * each descriptor (num_descs) */
const covt_stream_desc* covt_device_plan_descs_device(const covt_device_plan* plan);
const covt_stream_info* covt_device_plan_streams_device(const covt_device_plan* plan);
const int32_t* covt_device_plan_tile_status_device(const covt_device_plan* plan);
const uint32_t* covt_device_plan_order_device(const covt_device_plan* plan);
/* copies of the device arrays into host memory (any pointer may be NULL) */
int covt_device_plan_copy(const covt_device_plan* plan, covt_stream_info* streams, covt_stream_desc* descs,
                          int32_t* tile_status);
/* Geometry assembly from a device plan (covt_plan_geometry_columns / covt_plan_geometry_descs built on
 * the device, CovtParser.convertGeometryColumn's input): the first call of covt_device_plan_geometry
 * (or covt_device_plan_assemble) builds the geometry-column records and launch-ordered descriptors on
 * `hip_stream` -- the host plan's exactly -- and synchronises it; later calls return at once. */
int covt_device_plan_geometry(covt_device_plan* plan, void* hip_stream);
int64_t covt_device_plan_num_geometry_columns(const covt_device_plan* plan); /* 0 before geometry() */
int64_t covt_device_plan_assembly_bytes(const covt_device_plan* plan);
const covt_geom_desc* covt_device_plan_geometry_descs_device(const covt_device_plan* plan);
int covt_device_plan_geometry_copy(const covt_device_plan* plan, covt_geom_info* infos, covt_geom_desc* descs);
/* covt_assemble_geometry_device over the plan's geometry descriptors (built first if needed), after
 * covt_device_plan_decode on the same stream: d_asm covt_device_plan_assembly_bytes bytes, d_gres one
 * result per column in launch order (column c's at its covt_geom_info.desc_index). */
int covt_device_plan_assemble(covt_device_plan* plan, const uint8_t* d_decoded, const covt_stream_result* d_res,
                              uint8_t* d_asm, covt_geom_result* d_gres, void* hip_stream);
/* WKB columns from a device plan: the records and descriptors of covt_plan_wkb_columns /
 * covt_plan_wkb_descs, built on the device together with the geometry records (covt_device_plan_geometry;
 * the host plan's exactly); 0 / NULL before that call. */
int64_t covt_device_plan_wkb_bytes(const covt_device_plan* plan);
const covt_wkb_desc* covt_device_plan_wkb_descs_device(const covt_device_plan* plan);
int covt_device_plan_wkb_copy(const covt_device_plan* plan, covt_wkb_info* infos, covt_wkb_desc* descs);
/* covt_geometry_wkb_device over the plan's descriptors, after covt_device_plan_assemble on the same stream:
 * d_wkb covt_device_plan_wkb_bytes bytes, d_wres one result per column in launch order (column c's at its
 * covt_wkb_info.desc_index).  d_res is unused (the assembly results carry the source streams' statuses). */
int covt_device_plan_wkb(covt_device_plan* plan, const uint8_t* d_decoded, const covt_stream_result* d_res,
                         const uint8_t* d_asm, const covt_geom_result* d_gres, uint8_t* d_wkb,
                         covt_wkb_result* d_wres, void* hip_stream);
/* Bounding-box columns from a device plan: the records and descriptors of covt_plan_bbox_columns /
 * covt_plan_bbox_descs, built on the device next to the WKB records (covt_device_plan_geometry; the host
 * plan's exactly); 0 / NULL before that call. */
int64_t covt_device_plan_bbox_bytes(const covt_device_plan* plan);
const covt_bbox_desc* covt_device_plan_bbox_descs_device(const covt_device_plan* plan);
int covt_device_plan_bbox_copy(const covt_device_plan* plan, covt_bbox_info* infos, covt_bbox_desc* descs);
/* covt_geometry_bbox_device over the plan's descriptors, after covt_device_plan_assemble on the same stream:
 * d_bbox covt_device_plan_bbox_bytes bytes, d_bres one result per column in launch order (column c's at its
 * covt_bbox_info.desc_index). */
int covt_device_plan_bbox(covt_device_plan* plan, const uint8_t* d_asm, const covt_geom_result* d_gres,
                          uint8_t* d_bbox, covt_bbox_result* d_bres, void* hip_stream);
/* Measures columns from a device plan: the records and descriptors of covt_plan_measures_columns /
 * covt_plan_measures_descs, built on the device next to the bounding-box records (covt_device_plan_geometry;
 * the host plan's exactly); 0 / NULL before that call. */
int64_t covt_device_plan_measures_bytes(const covt_device_plan* plan);
const covt_measures_desc* covt_device_plan_measures_descs_device(const covt_device_plan* plan);
int covt_device_plan_measures_copy(const covt_device_plan* plan, covt_measures_info* infos, covt_measures_desc* descs);
/* covt_geometry_measures_device over the plan's descriptors, after covt_device_plan_assemble on the same
 * stream: d_measures covt_device_plan_measures_bytes bytes, d_mres one result per column in launch order
 * (column c's at its covt_measures_info.desc_index). */
int covt_device_plan_measures(covt_device_plan* plan, const uint8_t* d_decoded, const uint8_t* d_asm,
                              const covt_geom_result* d_gres, uint8_t* d_measures, covt_measures_result* d_mres,
                              void* hip_stream);
/* Select columns from a device plan: the records and descriptors of covt_plan_select_columns /
 * covt_plan_select_descs, built on the device next to the measures records (covt_device_plan_geometry; the host
 * plan's exactly); 0 / NULL before that call. */
int64_t covt_device_plan_select_bytes(const covt_device_plan* plan);
const covt_select_desc* covt_device_plan_select_descs_device(const covt_device_plan* plan);
int covt_device_plan_select_copy(const covt_device_plan* plan, covt_select_info* infos, covt_select_desc* descs);
/* covt_geometry_select_device over the plan's descriptors, after covt_device_plan_wkb and whatever wrote the
 * masks on the same stream: d_select covt_device_plan_select_bytes bytes, d_sres one result per column in
 * launch order (column c's at its covt_select_info.desc_index). */
int covt_device_plan_select(covt_device_plan* plan, const uint8_t* d_wkb, const covt_wkb_result* d_wres,
                            uint8_t* d_select, covt_select_result* d_sres, void* hip_stream);
/* Simplify columns from a device plan: the records and descriptors of covt_plan_simplify_columns /
 * covt_plan_simplify_descs and the retargeted geometry descriptors of covt_plan_simplified_geometry_descs, built
 * on the device next to the select records (covt_device_plan_geometry; the host plan's exactly); 0 / NULL
 * before that call. */
int64_t covt_device_plan_simplify_bytes(const covt_device_plan* plan);
const covt_simplify_desc* covt_device_plan_simplify_descs_device(const covt_device_plan* plan);
int covt_device_plan_simplify_copy(const covt_device_plan* plan, covt_simplify_info* infos, covt_simplify_desc* descs);
const covt_geom_desc* covt_device_plan_simplified_geometry_descs_device(const covt_device_plan* plan);
/* covt_geometry_simplify_device over the plan's descriptors, after covt_device_plan_assemble on the same
 * stream: d_simplify covt_device_plan_simplify_bytes bytes, d_gres_out one result per column in launch order. */
int covt_device_plan_simplify(covt_device_plan* plan, const uint8_t* d_decoded, const uint8_t* d_asm,
                              const covt_geom_result* d_gres, int32_t shift, const int32_t* d_shift,
                              uint8_t* d_simplify, covt_geom_result* d_gres_out, void* hip_stream);
/* MVT columns from a device plan: the records and descriptors of covt_plan_mvt_columns / covt_plan_mvt_descs,
 * built on the device next to the simplify records (the host plan's exactly); 0 / NULL before
 * covt_device_plan_geometry. */
int64_t covt_device_plan_mvt_bytes(const covt_device_plan* plan);
const covt_mvt_desc* covt_device_plan_mvt_descs_device(const covt_device_plan* plan);
int covt_device_plan_mvt_copy(const covt_device_plan* plan, covt_mvt_info* infos, covt_mvt_desc* descs);
/* covt_geometry_mvt_device over the plan's descriptors, after covt_device_plan_assemble (simplified != 0: after
 * covt_device_plan_simplify, d_asm / d_gres its buffer and results) on the same stream: d_mvt
 * covt_device_plan_mvt_bytes bytes, d_mvres one result per column in launch order. */
int covt_device_plan_mvt(covt_device_plan* plan, const uint8_t* d_decoded, const uint8_t* d_asm,
                         const covt_geom_result* d_gres, int32_t simplified, const covt_mvt_options* opts,
                         uint8_t* d_mvt, covt_mvt_result* d_mvres, void* hip_stream);
/* Property columns from a device plan made with COVT_PLAN_PROPERTIES in opts->flags: the records,
 * output layout and largest-first descriptors of covt_plan_property_columns / covt_plan_property_descs,
 * built on the device with the plan (the host plan's exactly); a plan without the flag has none. */
int64_t covt_device_plan_num_property_columns(const covt_device_plan* plan);
int64_t covt_device_plan_property_bytes(const covt_device_plan* plan);
const covt_prop_desc* covt_device_plan_property_descs_device(const covt_device_plan* plan);
int covt_device_plan_property_copy(const covt_device_plan* plan, covt_prop_info* infos, covt_prop_desc* descs);
/* covt_materialize_properties_device over the plan's property descriptors, after covt_device_plan_decode
 * on the same stream: d_props covt_device_plan_property_bytes bytes, d_pres one result per (sub)column in
 * descriptor order (column c's at its covt_prop_info.desc_index). */
int covt_device_plan_materialize(const covt_device_plan* plan, const uint8_t* d_in, const uint8_t* d_decoded,
                                 const covt_stream_result* d_res, uint8_t* d_props, covt_prop_result* d_pres,
                                 void* hip_stream);
/* the grouped decode launch over the plan's descriptors (covt_decode_streams_device_grouped):
 * d_out covt_device_plan_output_bytes bytes, d_res num_descs results (stream i's at its desc_index).
 * Asynchronous. */
int covt_device_plan_decode(const covt_device_plan* plan, const uint8_t* d_in, uint8_t* d_out,
                            covt_stream_result* d_res, void* hip_stream);

/* Library info */
const char* covt_version(void);
int covt_device_count(int32_t* n);

#ifdef __cplusplus
}
#endif
#endif /* COVT_H */

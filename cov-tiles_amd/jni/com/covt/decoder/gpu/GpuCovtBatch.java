package com.covt.decoder.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;

/**
 * Whole-tile batch decode on an AMD MI355X through libcovt's plan API (include/covt.h, "plan"):
 * the metadata of every tile is walked on the host (what CovtParser.decodeCovt does per layer,
 * CovtParser.java:53-133), then every Id and Geometry stream -- and with PLAN_PROPERTIES every
 * property column -- of the whole batch is decoded in one GPU launch.  Outputs land in direct
 * ByteBuffers (little-endian) at the offsets of {@link #streams()} / {@link #propertyColumns()},
 * so a Java caller reads them without copies; per-stream statuses are the include/covt.h codes.
 *
 * <p>Built with the JNI shim cov-tiles_amd/jni/covt_jni.cc (make -C cov-tiles_amd jni JAVA_HOME=...).
 */
public final class GpuCovtBatch implements AutoCloseable {
    static { System.loadLibrary("covt_jni"); }

    public static final int FORMAT_GENC = 0;     // COVT_FORMAT_GENC: the committed fixtures
    public static final int FORMAT_GEND = 1;     // COVT_FORMAT_GEND: what CovtParser.decodeCovt reads
    public static final int ID_FORMAT = 0;       // COVT_ID_FORMAT: 64-bit ids
    public static final int ID_JAVA = 1;         // COVT_ID_JAVA: CovtParser's 4-byte varint cap
    public static final int PLAN_PROPERTIES = 1; // COVT_PLAN_PROPERTIES
    /** Fields per row of {@link #streams()}: covt_stream_info in order (tile, layer, column_kind,
     * stream_type, encoding, column_type, num_values, byte_length, num_bits, op, elem_bytes,
     * desc_index, in_off, out_off, out_elems). */
    public static final int STREAM_FIELDS = 15;
    /** Fields per row of {@link #propertyColumns()}: covt_prop_info in order (tile, layer, column, type,
     * column_type, n_features, n_data, n_dict, lang, name_len, lang_len, dict_bytes, stream[3],
     * desc_index, name_off, lang_off, out_off[4]); name_off / lang_off index the batch input. */
    public static final int PROPERTY_FIELDS = 22;
    /** Fields per row of {@link #wkbColumns()}: covt_wkb_info in order (tile, layer, n_features,
     * desc_index, offsets_off, bytes_off, byte_cap); the offsets index the buffer of {@link #geometryWkb}. */
    public static final int WKB_FIELDS = 7;
    /** Fields per row of {@link #bboxColumns()}: covt_bbox_info in order (tile, layer, n_features,
     * desc_index, off); off indexes the buffer of {@link #geometryBbox}. */
    public static final int BBOX_FIELDS = 5;
    /** Fields per row of {@link #geometryBbox}: status, n_empty, then the column's extent xmin, ymin,
     * xmax, ymax as the bits of their doubles (Double.longBitsToDouble; NaN without a coordinate). */
    public static final int BBOX_RESULT_FIELDS = 6;
    /** Fields per row of {@link #measuresColumns()}: covt_measures_info in order (tile, layer, n_features,
     * desc_index, off); off indexes the buffer of {@link #geometryMeasures}. */
    public static final int MEASURES_FIELDS = 5;
    /** Coordinate reference systems of the georeferenced overloads (include/covt.h "Georeferenced
     * geometry"): tile pixels (the plain methods' output), EPSG:3857 metres, OGC:CRS84 lon/lat degrees. */
    public static final int CRS_TILE = 0, CRS_WEB_MERCATOR = 1, CRS_CRS84 = 2;

    private final ByteBuffer tiles;
    private final int numTiles;
    private long handle;

    public GpuCovtBatch(byte[][] tileBytes, int format, int idMode, int flags) {
        long total = 0;
        for (byte[] t : tileBytes) total += t.length;
        if (total > Integer.MAX_VALUE) throw new IllegalArgumentException("batch larger than 2 GiB");
        tiles = ByteBuffer.allocateDirect((int) total).order(ByteOrder.LITTLE_ENDIAN);
        long[] offsets = new long[tileBytes.length];
        long[] sizes = new long[tileBytes.length];
        for (int i = 0; i < tileBytes.length; i++) {
            offsets[i] = tiles.position();
            sizes[i] = tileBytes[i].length;
            tiles.put(tileBytes[i]);
        }
        tiles.clear();
        numTiles = tileBytes.length;
        handle = create(tiles, offsets, sizes, format, idMode, flags);
    }

    /** Per-tile walk status (0, or a negative COVT_ERR_*: that tile has no streams). */
    public int[] tileStatus() { return tileStatus(live(), numTiles); }

    public long numStreams() { return numStreams(live()); }

    /** Bytes {@link #decode} writes. */
    public long outputBytes() { return outputBytes(live()); }

    /** numStreams() rows of STREAM_FIELDS values, plan stream (tile) order. */
    public long[] streams() { return streams(live()); }

    /** Decodes every planned stream into {@code out} (direct, outputBytes() long); returns one
     * status per stream, plan order (COVT_OK = 0). */
    public int[] decode(ByteBuffer out) {
        if (!out.isDirect() || out.capacity() < outputBytes()) throw new IllegalArgumentException("output buffer");
        return decode(live(), tiles, out);
    }

    public long numPropertyColumns() { return numPropertyColumns(live()); }

    /** Bytes {@link #properties} writes. */
    public long propertyBytes() { return propertyBytes(live()); }

    /** numPropertyColumns() rows of PROPERTY_FIELDS values, tile order. */
    public long[] propertyColumns() { return propertyColumns(live()); }

    /** Decode + property materialization into {@code out} (direct, propertyBytes() long); returns
     * (status, n_valid) per property column, tile order. */
    public int[] properties(ByteBuffer out) {
        if (!out.isDirect() || out.capacity() < propertyBytes()) throw new IllegalArgumentException("output buffer");
        return properties(live(), tiles, out);
    }

    /** Bytes {@link #geometryWkb} writes. */
    public long wkbBytes() { return wkbBytes(live()); }

    /** One row of WKB_FIELDS values per geometry column, tile order. */
    public long[] wkbColumns() { return wkbColumns(live()); }

    /** Decode + geometry assembly + WKB serialization into {@code out} (direct, wkbBytes() long): per
     * column an int32 offsets array (n_features + 1, little-endian) at offsets_off and the features' ISO
     * WKB values back to back at bytes_off -- feature i is bytes [offsets[i], offsets[i + 1]), ready for
     * {@code new WKBReader().read(bytes)}.  Returns (status, n_bytes) per column, tile order. */
    public long[] geometryWkb(ByteBuffer out) {
        if (!out.isDirect() || out.capacity() < wkbBytes()) throw new IllegalArgumentException("output buffer");
        return geometryWkb(live(), tiles, out);
    }

    /** {@link #geometryWkb(ByteBuffer)} with every coordinate in {@code crs} instead of tile pixels: the
     * container does not hold a tile's address, so {@code tileZxy} gives z, x, y of every tile of the batch
     * (3 per tile, tile order).  Byte counts, offsets and the returned rows are those of the plain method;
     * Web Mercator coordinates and longitudes are bit-exact IEEE-754 evaluations of the header's formulas.
     * A wrong array length or an invalid address throws IllegalArgumentException. */
    public long[] geometryWkb(ByteBuffer out, int crs, int[] tileZxy) {
        if (!out.isDirect() || out.capacity() < wkbBytes()) throw new IllegalArgumentException("output buffer");
        return geometryWkbProjected(live(), tiles, out, crs, addresses(tileZxy), numTiles);
    }

    private long[] addresses(int[] tileZxy) {
        if (tileZxy == null || tileZxy.length != 3 * numTiles) throw new IllegalArgumentException("tileZxy: z, x, y per tile");
        long[] a = new long[tileZxy.length];
        for (int i = 0; i < a.length; i++) a[i] = tileZxy[i];
        return a;
    }

    /** Bytes {@link #geometryBbox} writes. */
    public long bboxBytes() { return bboxBytes(live()); }

    /** One row of BBOX_FIELDS values per geometry column, tile order. */
    public long[] bboxColumns() { return bboxColumns(live()); }

    /** Decode + geometry assembly + bounding boxes into {@code out} (direct, bboxBytes() long): per column,
     * at off, four little-endian float64 arrays of n_features values back to back -- xmin, ymin, xmax, ymax,
     * the GeoParquet bbox covering column of the WKB column of {@link #geometryWkb}; a feature without a
     * coordinate holds NaN in all four.  Returns BBOX_RESULT_FIELDS values per column, tile order. */
    public long[] geometryBbox(ByteBuffer out) {
        if (!out.isDirect() || out.capacity() < bboxBytes()) throw new IllegalArgumentException("output buffer");
        return geometryBbox(live(), tiles, out);
    }

    /** {@link #geometryBbox(ByteBuffer)} in {@code crs} (see {@link #geometryWkb(ByteBuffer, int, int[])}): the
     * boxes and the extents of the returned rows are in that CRS, so the column prunes across tiles. */
    public long[] geometryBbox(ByteBuffer out, int crs, int[] tileZxy) {
        if (!out.isDirect() || out.capacity() < bboxBytes()) throw new IllegalArgumentException("output buffer");
        return geometryBboxProjected(live(), tiles, out, crs, addresses(tileZxy), numTiles);
    }

    /** Bytes {@link #geometryMeasures} writes. */
    public long measuresBytes() { return measuresBytes(live()); }

    /** One row of MEASURES_FIELDS values per geometry column, tile order. */
    public long[] measuresColumns() { return measuresColumns(live()); }

    /** Decode + geometry assembly + measures into {@code out} (direct, measuresBytes() long): per column, at
     * off, little-endian area[n_features] and length[n_features] float64, then num_coords[n_features] int32 --
     * what JTS getArea(), getLength() and getNumPoints() give for the feature of {@link #geometryWkb}, in tile
     * pixels.  Returns one status per column, tile order. */
    public long[] geometryMeasures(ByteBuffer out) {
        if (!out.isDirect() || out.capacity() < measuresBytes()) throw new IllegalArgumentException("output buffer");
        return geometryMeasures(live(), tiles, out);
    }

    @Override
    public void close() {
        if (handle != 0) destroy(handle);
        handle = 0;
    }

    private long live() {
        if (handle == 0) throw new IllegalStateException("closed");
        return handle;
    }

    private static native long create(ByteBuffer tiles, long[] offsets, long[] sizes, int format, int idMode, int flags);
    private static native void destroy(long plan);
    private static native int[] tileStatus(long plan, int numTiles);
    private static native long numStreams(long plan);
    private static native long outputBytes(long plan);
    private static native long[] streams(long plan);
    private static native int[] decode(long plan, ByteBuffer tiles, ByteBuffer out);
    private static native long numPropertyColumns(long plan);
    private static native long propertyBytes(long plan);
    private static native long[] propertyColumns(long plan);
    private static native int[] properties(long plan, ByteBuffer tiles, ByteBuffer out);
    private static native long wkbBytes(long plan);
    private static native long[] wkbColumns(long plan);
    private static native long[] geometryWkb(long plan, ByteBuffer tiles, ByteBuffer out);
    private static native long bboxBytes(long plan);
    private static native long[] bboxColumns(long plan);
    private static native long[] geometryBbox(long plan, ByteBuffer tiles, ByteBuffer out);
    private static native long measuresBytes(long plan);
    private static native long[] measuresColumns(long plan);
    private static native long[] geometryMeasures(long plan, ByteBuffer tiles, ByteBuffer out);
    // (names of their own: an overloaded native method would need the signature-mangled symbol names)
    private static native long[] geometryWkbProjected(long plan, ByteBuffer tiles, ByteBuffer out, int crs,
                                                      long[] tileZxy, int numTiles);
    private static native long[] geometryBboxProjected(long plan, ByteBuffer tiles, ByteBuffer out, int crs,
                                                       long[] tileZxy, int numTiles);
}

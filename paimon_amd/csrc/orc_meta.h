// Host-side ORC file-structure reader (protobuf wire format): postscript,
// footer, stripe footers, stream locations. Replaces, for this path, the
// stripe planning the reference delegates to orc-core 1.9.8
// (format/orc/OrcReaderFactory.java:108-171 + vendored
// org.apache.orc.impl.RecordReaderImpl overrides). Decode arithmetic
// (RLEv2 / byte-RLE / boolean-RLE) runs on the GPU (kernels.hip); this
// parser only locates streams; compressed files (zlib / snappy / zstd)
// have their footers inflated here and their streams at staging.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace pmh {

enum OrcTypeKind {
    ORC_BOOLEAN = 0,
    ORC_BYTE = 1,
    ORC_SHORT = 2,
    ORC_INT = 3,
    ORC_LONG = 4,
    ORC_FLOAT = 5,
    ORC_DOUBLE = 6,
    ORC_STRING = 7,
    ORC_TIMESTAMP = 9,  // relative to 2015-01-01 in the WRITER's timezone
    ORC_STRUCT = 12,
    ORC_DECIMAL = 14,
    ORC_DATE = 15,      // signed RLEv2 days since 1970-01-01
    ORC_TIMESTAMP_INSTANT = 18,  // timestamp with local time zone: UTC
};

enum OrcStreamKind {
    ORC_STREAM_PRESENT = 0,
    ORC_STREAM_DATA = 1,
    ORC_STREAM_LENGTH = 2,
    ORC_STREAM_DICTIONARY = 3,
    ORC_STREAM_SECONDARY = 5,  // decimal: per-value scale, signed RLEv2;
                               // timestamp: nanoseconds, unsigned RLEv2
};

// StripeFooter.writerTimezone names UTC (TIMESTAMP columns of any other
// zone are refused at staging): empty, "UTC" or "GMT".
bool orc_timezone_is_utc(const std::string &tz);

struct OrcStream {
    int kind = 0;
    int column = 0;
    int64_t length = 0;
    int64_t offset = 0;  // absolute file offset
};

struct OrcStripe {
    int64_t offset = 0;
    int64_t index_length = 0;
    int64_t data_length = 0;
    int64_t footer_length = 0;
    int64_t num_rows = 0;
    std::vector<OrcStream> streams;
    std::vector<int> encodings;  // per column id
    std::string writer_timezone;  // StripeFooter.writerTimezone ("" = none)
};

struct OrcFileMeta {
    int64_t num_rows = 0;
    int compression = 0;  // CompressionKind: 0 NONE, 1 ZLIB, 5 ZSTD (v1 set)
    int64_t compression_block_size = 0;
    std::vector<std::string> column_names;  // flat struct; col id = idx + 1
    std::vector<int> column_kinds;
    // Type.precision / Type.scale (DECIMAL columns; 0 elsewhere)
    std::vector<int> column_precisions;
    std::vector<int> column_scales;
    std::vector<OrcStripe> stripes;
    std::string error;
    bool ok() const { return error.empty(); }
};

OrcFileMeta parse_orc_meta(const uint8_t *data, int64_t size);

bool is_orc_file(const uint8_t *data, int64_t size);

const OrcStream *orc_find_stream(const OrcStripe &st, int column, int kind);

}  // namespace pmh

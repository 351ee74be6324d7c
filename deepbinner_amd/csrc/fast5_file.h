// fast5_file.h - a fast5 file as the loaders see it: which reads it holds, each read's id and
// Signal, and the attributes a one-read copy of a read carries.
#ifndef DEEPBINNER_FAST5_FILE_H
#define DEEPBINNER_FAST5_FILE_H

#include "fast5_signal.h"

namespace {

struct ReadEntry {
    uint64_t group_addr = 0;          // the group that holds Signal and read_id (".../Raw")
    uint64_t read_group_addr = 0;     // multi-read containers: /read_<id> itself (0 otherwise)
    bool resolved = false;
    std::string read_id;
    SignalInfo signal;
};

class Fast5 : public SignalFile {
  public:
    using SignalFile::SignalFile;

    // ---- what the C ABI needs ----------------------------------------------------------------
    void parse() {
        parse_superblock();
        find_reads();
    }
    int layout() const { return layout_; }
    int64_t n_reads() const { return (int64_t)reads_.size(); }

    const ReadEntry& read(int64_t index) {
        if (index < 0 || index >= (int64_t)reads_.size()) throw std::out_of_range("read index");
        ReadEntry& r = reads_[(size_t)index];
        if (!r.resolved) {
            const std::vector<Msg> msgs = object_header(r.group_addr);
            if (!find_string_attribute(msgs, "read_id", &r.read_id))
                throw std::out_of_range("read group without read_id");
            const std::map<std::string, uint64_t> links = group_links(msgs);
            auto it = links.find("Signal");
            if (it == links.end()) throw std::out_of_range("read group without Signal");
            r.signal = signal_info(it->second);
            r.resolved = true;
        }
        return r;
    }

    // What a one-read copy of read `index` carries beside its Signal (ont_fast5_api's
    // multi_to_single_fast5, the tool the reference runs - realtime.py:183-190 - copies the same):
    // the attributes of the read group, of Raw, and of channel_id / tracking_id / context_tags.
    struct ReadMeta {
        Attrs read, raw, group[3];
        bool has[3] = {false, false, false};
    };
    static const char* meta_group_name(int k) {
        static const char* const names[3] = {"channel_id", "tracking_id", "context_tags"};
        return names[k];
    }
    void read_metadata(int64_t index, ReadMeta* out) {
        const ReadEntry& r = read(index);
        out->raw = attributes(r.group_addr);
        if (r.read_group_addr == 0) return;
        out->read = attributes(r.read_group_addr);
        const std::map<std::string, uint64_t> links = group_links(object_header(r.read_group_addr));
        for (int k = 0; k < 3; ++k) {
            auto it = links.find(meta_group_name(k));
            if (it == links.end()) continue;
            out->group[k] = attributes(it->second);
            out->has[k] = true;
        }
    }

  private:
    int layout_ = F5_LAYOUT_NONE;
    std::vector<ReadEntry> reads_;

    // ---- which reads the file holds (load_fast5s.py:29-43) ---------------------------------------
    void find_reads() {
        const std::map<std::string, uint64_t> root = group_links(object_header(root_addr_));
        auto raw = root.find("Raw");
        if (raw != root.end()) {   // older format: exactly one read under /Raw/Reads
            const std::map<std::string, uint64_t> raw_links = group_links(object_header(raw->second));
            auto reads = raw_links.find("Reads");
            if (reads == raw_links.end()) throw std::out_of_range("no /Raw/Reads");
            const std::map<std::string, uint64_t> children = group_links(object_header(reads->second));
            if (children.empty()) throw std::out_of_range("empty /Raw/Reads");
            ReadEntry e;
            e.group_addr = children.begin()->second;
            reads_.push_back(e);
            layout_ = F5_LAYOUT_SINGLE_OLD;
            return;
        }
        for (const auto& kv : root) {
            if (kv.first.compare(0, 5, "read_") != 0) continue;
            const std::map<std::string, uint64_t> links = group_links(object_header(kv.second));
            auto r = links.find("Raw");
            if (r == links.end()) throw std::out_of_range("read group without Raw");
            ReadEntry e;
            e.group_addr = r->second;
            e.read_group_addr = kv.second;
            reads_.push_back(e);
        }
        layout_ = reads_.empty() ? F5_LAYOUT_NONE
                                 : (reads_.size() == 1 ? F5_LAYOUT_SINGLE_NEW : F5_LAYOUT_MULTI);
    }
};

}  // namespace

#endif  // DEEPBINNER_FAST5_FILE_H

// read_source.h -- the sequences of a .db, .dam or FASTX input, one after the other and pass after pass (kprof,
// genome2class).  Plain C++; no device code.
#pragma once
#include <cerrno>
#include "host_io.h"
#include "dazz_db.h"
#include "class_record.h"

struct Source
  { std::string path;
    bool is_db = false, is_dam = false;
    DazzDB db;
    FastxReader *fx = nullptr;
    int next_db = 0;
    std::string seq, header;
    bool find(const std::string &name, std::string *dir, std::string *root)    // false: none of the ten forms exists
    { const int idx = find_source(name,dir,root);
      if (idx == 10) return false;
      path = *dir+"/"+*root+EXT[idx];
      is_db = idx <= 1; is_dam = idx == 1;
      return true;
    }
    void open()
    { if (is_db) { db.open(path,is_dam); return; }
      fx = new FastxReader(path.c_str());
      if (!fx->f) die("%s: Cannot open %s [errno=%d]\n",PROG,path.c_str(),errno);
    }
    void rewind()                                                 // starts the next pass
    { next_db = 0;
      if (is_db) return;
      delete fx;
      fx = nullptr;
      open();
    }
    bool next()                                                   // the next sequence into seq, its .class header into header
    { if (is_db)
        { if (next_db >= db.nreads) return false;
          header = db.header(next_db);
          db.load(next_db++,seq);
          return true;
        }
      if (fx->next() < 0)
        { if (fx->bad_qual) die("%s: %s: a quality string is not as long as its sequence\n",PROG,path.c_str());
          return false;
        }
      seq.swap(fx->seq);
      header = fastx_class_header(*fx);
      return true;
    }
  };

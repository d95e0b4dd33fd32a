"""The rules of lbm-asynchronous_amd/Makefile as the tests read them: a target's line with the variables of its
prerequisites written out, so "the library is rebuilt when this header changes" is asked of what make sees."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rule_line(target):
    """the line `target: prerequisites` (target with its colon), every $(NAME) in it replaced by NAME's value"""
    text = open(os.path.join(ROOT, "lbm-asynchronous_amd", "Makefile")).read().replace("\\\n", " ")
    values = dict(re.findall(r"^(\w+)\s*\??=\s*(.*)$", text, flags=re.M))
    line = next(l for l in text.splitlines() if l.startswith(target))
    return re.sub(r"\$\((\w+)\)", lambda m: values[m.group(1)], line)

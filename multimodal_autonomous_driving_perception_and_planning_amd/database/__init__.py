"""Storage for auto-tagging results (src/database of the reference)."""
from .tag_database import QueryResult, TagDatabase, tag_log_session

__all__ = ["TagDatabase", "QueryResult", "tag_log_session"]
